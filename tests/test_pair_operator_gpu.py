"""
GPU tests of the pair-list operator: ``k_pairs_apply`` / ``k_pairs_strain`` of csrc/pair_operator.hip through
``sc_dev_pairs_apply_f64`` / ``sc_dev_pairs_strain_f64``, :class:`springcraft_amd.PairOperator`, the model functions
``nma.deformation_energy`` / ``nma.spring_strain`` and the RTB consumers ``residuals`` / ``deformation_energy`` /
``spring_strain``.

Reference: :func:`restate`, NumPy on the three formulas, for the pair list of ``compute_hessian`` and the constants of the
force field's own ``force_constant()`` on NumPy's squared distances; and the dense product with the package's own
``compute_hessian`` / ``compute_kirchhoff`` matrix, which ties the operator to the matrix the solvers decompose.

Structures: seeded random-walk chains with 3.8 A steps.  N = 1 (no pair); N = 40 under ``InvariantForceField(7.0)`` with atom
17 moved 100 A away (an atom without pairs); N = 66 and N = 131 under ``HinsenForceField()`` (no cutoff: 65 and 130
neighbours per atom, two and three lane chunks of 64); N = 300 under ``InvariantForceField(8.0)`` (75 workgroups).  Each
with and without masses ``RandomState(5).uniform(50, 200, N)``; dim 1 at N = 40 and N = 66.  Rows: q in {1, 4, 5, 9}, the first
q of nine standard-normal rows per structure (a row's result does not depend on the others, so one reference serves).

Tolerances, derived.  With ``u = t x`` per atom, every term of atom i's sum for Y is at most ``gamma_p (|u_i|_1 + |u_j|_1)``
in magnitude and carries a few roundings of its own; a float64 sum of fewer than 1000 such terms errs by less than 1e-13
of ``B_i = sum_p gamma_p (|u_i|_1 + |u_j|_1)``.  Gate: ``|Y - Y_ref| <= 1e-12 t_i B_i`` elementwise, for the restatement and
for the dense product (at most 900 terms per row here, each within the same magnitudes).  For E the same with the terms
squared, ``C_i = 1/2 sum_p gamma_p (|u_i|_1 + |u_j|_1)^2``; for one spring's strain ``1e-12 gamma_p (|u_i|_1 + |u_j|_1)^2``.
Sums over atoms: ``sum_i E[i]`` errs by at most ``1e-12 sum_i C_i`` and ``<x, Y>`` by ``1e-12 sum_i |u_i|_1 B_i`` plus the
rounding of a dot product of 3N such terms, which the same figure covers; the gate of the energy / Rayleigh identity
is 1e-12 times the sum of the two, and of the strain total (2 x^T H x, every spring twice) twice that.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QS = (1, 4, 5, 9)
ISOLATED = 17


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def chain(n, seed):
    rng = np.random.RandomState(seed)
    step = rng.standard_normal((n, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1)[:, None]
    return np.cumsum(step, axis=0)


def masses_of(n):
    return np.random.RandomState(5).uniform(50, 200, n)


def structure(sc, name):
    if name == "n1":
        return chain(1, 1), sc.InvariantForceField(7.0)
    if name == "n40":
        return chain(40, 2), sc.InvariantForceField(7.0)
    if name == "n40iso":
        coord = chain(40, 2)
        coord[ISOLATED] += 100.0
        return coord, sc.InvariantForceField(7.0)
    if name == "n66":
        return chain(66, 3), sc.HinsenForceField()
    if name == "n131":
        return chain(131, 4), sc.HinsenForceField()
    if name == "n300":
        return chain(300, 5), sc.InvariantForceField(8.0)
    raise KeyError(name)


def network(sc, coord, ff):
    """(pairs, gamma): the ordered pair list of the package and the force field's constants on NumPy's distances."""
    if len(coord) == 1:
        return np.empty((0, 2), dtype=np.int64), np.empty(0)
    _, pairs = sc.compute_kirchhoff(coord, ff)
    d = coord[pairs[:, 1]] - coord[pairs[:, 0]]
    gamma = np.asarray(ff.force_constant(pairs[:, 0], pairs[:, 1], (d * d).sum(axis=1)), dtype=np.float64)
    return pairs, gamma


def restate(coord, pairs, gamma, scale, x, dim):
    """
    The three formulas in NumPy for the rows ``x`` (q, dim N): Y (q, dim N), E (q, N), S (q, k), and the magnitudes of the
    tolerances, B (q, N), Cb (q, N) and per spring Sb (q, k).
    """
    n, q = len(coord), len(x)
    i, j = pairs[:, 0], pairs[:, 1]
    t = np.ones(n) if scale is None else scale
    if dim == 3:
        u = x.reshape(q, n, 3) * t[None, :, None]
        d = coord[j] - coord[i]
        nvec = d / np.sqrt((d * d).sum(axis=1))[:, None]
        e = ((u[:, i] - u[:, j]) * nvec[None]).sum(axis=2)
        term = (gamma * e)[:, :, None] * nvec[None]
        l1 = np.abs(u).sum(axis=2)
    else:
        u = x * t[None, :]
        e = u[:, i] - u[:, j]
        term = (gamma * e)[:, :, None]
        l1 = np.abs(u)
    S = gamma * e * e
    Y = np.zeros((q, n, dim))
    E = np.zeros((q, n))
    B = np.zeros((q, n))
    Cb = np.zeros((q, n))
    mag = l1[:, i] + l1[:, j]
    Sb = gamma * mag * mag
    for r in range(q):
        np.add.at(Y[r], i, term[r])
        np.add.at(E[r], i, 0.5 * S[r])
        np.add.at(B[r], i, gamma * mag[r])
        np.add.at(Cb[r], i, 0.5 * Sb[r])
    Y *= t[None, :, None]
    return {"Y": Y.reshape(q, dim * n), "E": E, "S": S, "B": B * t[None, :], "C": Cb, "Sb": Sb, "l1": l1}


CASES = [(name, masses, 3) for name in ("n1", "n40iso", "n66", "n131", "n300") for masses in (False, True)]
CASES += [(name, masses, 1) for name in ("n40iso", "n66") for masses in (False, True)]
CASE_IDS = [f"{name}-{'mass' if masses else 'plain'}-dim{dim}" for name, masses, dim in CASES]

_cache = {}


def case_of(sc, torch, key):
    """Everything a case's tests share, built once: the operator, nine rows, the restatement and the device results."""
    if key not in _cache:
        name, masses, dim = key
        coord, ff = structure(sc, name)
        n = len(coord)
        mass = masses_of(n) if masses else None
        pairs, gamma = network(sc, coord, ff)
        x = np.random.RandomState(11).standard_normal((9, dim * n))
        scale = None if mass is None else 1.0 / np.sqrt(mass)
        op = sc.PairOperator(coord, ff, dim=dim, masses=mass)
        xd = torch.from_numpy(x).cuda()
        y, e = op.apply_energy(xd)
        _cache[key] = {"coord": coord, "ff": ff, "n": n, "mass": mass, "scale": scale, "pairs": pairs, "gamma": gamma,
                       "name": name, "x": x, "xd": xd, "op": op, "ref": restate(coord, pairs, gamma, scale, x, dim), "dim": dim,
                       "y": y, "e": e, "yh": y.cpu().numpy(), "eh": e.cpu().numpy()}
    return _cache[key]


@pytest.fixture(params=CASES, ids=CASE_IDS)
def case(request, sc, torch):
    return case_of(sc, torch, request.param)


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def test_operator_holds_the_package_pair_list(case):
    op = case["op"]
    assert np.array_equal(op.pairs, case["pairs"])
    assert op.n_pairs == len(case["pairs"]) and op.n_atoms == case["n"] and op.dim == case["dim"]
    assert np.allclose(op.gamma, case["gamma"], rtol=1e-14, atol=0)
    assert np.array_equal(op.springs, case["pairs"][case["pairs"][:, 0] < case["pairs"][:, 1]])


def test_apply_and_energy_match_the_restatement(case):
    ref, dim = case["ref"], case["dim"]
    err_y = np.abs(case["yh"] - ref["Y"])
    tol_y = 1e-12 * np.repeat(ref["B"], dim, axis=1)
    err_e = np.abs(case["eh"] - ref["E"])
    tol_e = 1e-12 * ref["C"]
    print(f"Y: max err / tol {np.max(err_y / np.where(tol_y > 0, tol_y, 1)):.3e}; "
          f"E: {np.max(err_e / np.where(tol_e > 0, tol_e, 1)):.3e}")
    assert np.all(err_y <= tol_y)
    assert np.all(err_e <= tol_e)
    assert np.all(case["eh"] >= 0)


@pytest.mark.parametrize("q", QS)
def test_every_row_count_gives_the_same_bits(case, torch, q):
    op, xd = case["op"], case["xd"]
    y, e = op.apply_energy(xd[:q])
    assert y.shape == (q, case["dim"] * case["n"]) and e.shape == (q, case["n"])
    assert torch.equal(bits(y), bits(case["y"][:q])) and torch.equal(bits(e), bits(case["e"][:q]))
    # apply and energy alone are the same sums as the joint pass
    assert torch.equal(bits(op.apply(xd[:q])), bits(y)) and torch.equal(bits(op.energy(xd[:q])), bits(e))
    for r in range(q):
        y1, e1 = op.apply_energy(xd[r: r + 1])
        assert torch.equal(bits(y1[0]), bits(y[r])) and torch.equal(bits(e1[0]), bits(e[r]))
    # a single vector in, a single vector out; a NumPy array is taken as well
    v = op.apply(case["x"][q - 1])
    assert v.shape == (case["dim"] * case["n"],) and torch.equal(bits(v), bits(y[q - 1]))


def test_two_calls_agree_and_a_nan_row_stays_alone(case, torch):
    op, xd, n, dim = case["op"], case["xd"], case["n"], case["dim"]
    y, e = op.apply_energy(xd)
    assert torch.equal(bits(y), bits(case["y"])) and torch.equal(bits(e), bits(case["e"]))
    bad = xd.clone()
    bad[2] = float("nan")
    yb, eb = op.apply_energy(bad)
    keep = [r for r in range(len(xd)) if r != 2]
    assert torch.equal(bits(yb[keep]), bits(y[keep])) and torch.equal(bits(eb[keep]), bits(e[keep]))
    has_pairs = torch.from_numpy(np.bincount(case["pairs"][:, 0], minlength=n) > 0).cuda()
    assert bool(torch.isnan(eb[2][has_pairs]).all()) and bool(torch.isnan(yb[2].view(n, dim)[has_pairs]).all())
    assert bool((eb[2][~has_pairs] == 0).all()) and bool((yb[2].view(n, dim)[~has_pairs] == 0).all())


def test_an_atom_without_pairs_gives_exact_zeros(case):
    n, dim = case["n"], case["dim"]
    lonely = np.nonzero(np.bincount(case["pairs"][:, 0], minlength=n) == 0)[0]
    y = case["yh"].reshape(-1, n, dim)
    assert np.all(y[:, lonely] == 0.0) and np.all(case["eh"][:, lonely] == 0.0)
    assert not np.any(np.signbit(y[:, lonely])) and not np.any(np.signbit(case["eh"][:, lonely]))
    if case["name"] == "n40iso":
        assert list(lonely) == [ISOLATED]
    elif case["name"] == "n1":
        assert list(lonely) == [0] and case["op"].n_pairs == 0
    else:
        assert len(lonely) == 0


def test_energy_sums_to_the_rayleigh_quotient_and_the_strain_to_twice_it(case, torch):
    op, xd, ref = case["op"], case["xd"], case["ref"]
    total = case["e"].sum(dim=1).cpu().numpy()
    xx = (case["x"] * case["x"]).sum(axis=1)
    quad = op.rayleigh(xd).cpu().numpy() * xx
    tol = 1e-12 * (ref["C"].sum(axis=1) + (ref["l1"] * ref["B"] / (1.0 if case["scale"] is None else case["scale"])).sum(axis=1))
    print(f"energy vs rayleigh: max err / tol {np.max(np.abs(total - quad) / np.where(tol > 0, tol, 1)):.3e}")
    assert np.all(np.abs(total - quad) <= tol)
    assert np.all(np.abs(total - ref["E"].sum(axis=1)) <= tol)
    every = op.strain(xd, np.arange(op.n_pairs))
    assert every.shape == (9, op.n_pairs)
    assert np.all(np.abs(every.sum(dim=1).cpu().numpy() - 2 * total) <= 2 * tol)
    assert np.all(np.abs(every.cpu().numpy() - ref["S"]) <= 1e-12 * ref["Sb"])
    # a single row: 0-d results
    assert op.rayleigh(xd[0]).shape == () and op.residual(1.0, xd[0]).shape == ()


def test_default_strain_is_every_spring_once(case, torch):
    op, xd, ref = case["op"], case["xd"], case["ref"]
    rows = np.nonzero(case["pairs"][:, 0] < case["pairs"][:, 1])[0]
    for q in QS:
        s = op.strain(xd[:q])
        assert s.shape == (q, len(op.springs)) == (q, len(rows))
        assert np.all(np.abs(s.cpu().numpy() - ref["S"][:q, rows]) <= 1e-12 * ref["Sb"][:q, rows])
    assert op.strain(xd[0]).shape == (len(rows),)
    if len(rows):
        # both directions of a spring store the same
        back = np.nonzero(case["pairs"][:, 0] > case["pairs"][:, 1])[0]
        order = np.lexsort((case["pairs"][back, 0], case["pairs"][back, 1]))
        assert np.array_equal(case["pairs"][back[order]][:, ::-1], case["pairs"][rows])
        assert torch.equal(bits(op.strain(xd, back[order])), bits(op.strain(xd)))


def test_a_pair_index_out_of_range_gives_a_nan_column(case, torch):
    op, xd = case["op"], case["xd"]
    k = op.n_pairs
    idx = np.array([0, k, 1, -1, k + 12345, min(2, max(k - 1, 0))], dtype=np.int64)
    s = op.strain(xd[:5], idx)
    assert s.shape == (5, 6)
    inside = (idx >= 0) & (idx < k)
    assert bool(torch.isnan(s[:, torch.from_numpy(~inside).cuda()]).all())
    if inside.any():
        good = s[:, torch.from_numpy(inside).cuda()]
        assert bool(torch.isfinite(good).all())
        assert torch.equal(bits(good), bits(op.strain(xd[:5], idx[inside])))


def test_residual_is_the_norm_of_the_defect(case, torch):
    op, xd = case["op"], case["xd"]
    w = np.linspace(-1.0, 2.0, 9)
    r = op.residual(w, xd).cpu().numpy()
    ref = np.linalg.norm(case["yh"] - w[:, None] * case["x"], axis=1)
    assert r.shape == (9,) and np.allclose(r, ref, rtol=1e-13, atol=0)
    assert np.allclose(op.residual(0.5, xd).cpu().numpy(), np.linalg.norm(case["yh"] - 0.5 * case["x"], axis=1), rtol=1e-13)
    with pytest.raises(ValueError, match="eigenvalues"):
        op.residual(w[:4], xd)
    with pytest.raises(ValueError, match="Expected rows"):
        op.apply(np.zeros(case["dim"] * case["n"] + 1))


DENSE = [c for c in CASES if c[0] != "n1"]


@pytest.mark.parametrize("key", DENSE, ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] != "n1"])
def test_product_matches_the_dense_matrix(sc, torch, key):
    case = case_of(sc, torch, key)
    dim = case["dim"]
    h = (sc.compute_hessian if dim == 3 else sc.compute_kirchhoff)(case["coord"], case["ff"])[0]
    if case["scale"] is not None:
        s = np.repeat(case["scale"], dim)
        h = h * np.outer(s, s)
    dense = case["x"] @ h.T
    err = np.abs(case["yh"] - dense)
    tol = 1e-12 * np.repeat(case["ref"]["B"], dim, axis=1)
    print(f"dense: max err / tol {np.max(err / np.where(tol > 0, tol, 1)):.3e}")
    assert np.all(err <= tol)


def test_from_pairs_adopts_host_arrays_and_cuda_tensors(sc, torch):
    case = case_of(sc, torch, ("n66", True, 3))
    op = case["op"]
    host = sc.PairOperator.from_pairs(case["coord"], op.pairs, op.gamma, inv_sqrt_mass=case["scale"])
    dev = sc.PairOperator.from_pairs(torch.from_numpy(case["coord"]).cuda(), torch.from_numpy(op.pairs).cuda(),
                                     torch.from_numpy(op.gamma).cuda(), inv_sqrt_mass=torch.from_numpy(case["scale"]).cuda())
    for other in (host, dev):
        y, e = other.apply_energy(case["xd"])
        assert torch.equal(bits(y), bits(case["y"])) and torch.equal(bits(e), bits(case["e"]))
        assert np.array_equal(other.springs, op.springs)
    assert dev._pairs.data_ptr() != op._pairs.data_ptr()
    flipped = op.gamma.copy()
    flipped[3] *= 2
    with pytest.raises(ValueError, match="asymmetric"):
        sc.PairOperator.from_pairs(case["coord"], op.pairs, flipped)
    # dim 1 needs no coordinates
    g1 = case_of(sc, torch, ("n66", False, 1))
    bare = sc.PairOperator.from_pairs(None, g1["op"].pairs, g1["op"].gamma, dim=1, n_atoms=66)
    assert torch.equal(bits(bare.apply(g1["xd"])), bits(g1["y"]))
    with pytest.raises(ValueError, match="coordinates"):
        sc.PairOperator.from_pairs(None, op.pairs, op.gamma, dim=3, n_atoms=66)


def test_invalid_arguments_are_refused_before_a_launch(sc, torch):
    from springcraft_amd import _hip

    case = case_of(sc, torch, ("n40iso", False, 3))
    op, L = case["op"], _hip.lib()
    n, k, q = op.n_atoms, op.n_pairs, 2
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    x = case["xd"][:q].contiguous()
    y = torch.full((q, 3 * n), 7.0, dtype=torch.float64, device="cuda")
    e = torch.full((q, n), 7.0, dtype=torch.float64, device="cuda")

    def apply(coord=op._coord, n_atoms=n, dim=3, pairs=op._pairs, kk=k, gamma=op._gamma, start=op._row_start, rows=x,
              qq=q, out_y=y, out_e=e):
        return L.sc_dev_pairs_apply_f64(op.ctx.handle, p(coord), n_atoms, dim, p(pairs), kk, p(gamma), p(start), None,
                                        p(rows), qq, p(out_y), p(out_e))

    bad = _hip.SC_ERR_INVALID_ARG
    assert apply(out_y=None, out_e=None) == bad
    assert apply(dim=2) == bad and apply(dim=0) == bad
    assert apply(coord=None) == bad
    assert apply(n_atoms=0) == bad and apply(n_atoms=-3) == bad
    assert apply(kk=-1) == bad and apply(qq=-1) == bad
    assert apply(pairs=None) == bad and apply(gamma=None) == bad and apply(start=None) == bad and apply(rows=None) == bad
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((e == 7.0).all()), "a refused call wrote to its outputs"
    # valid corner cases: no rows; no pairs with NULL pair arrays (zeros)
    assert apply(qq=0, rows=None) == _hip.SC_OK
    assert apply(kk=0, pairs=None, gamma=None, start=None) == _hip.SC_OK
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and bool((e == 0.0).all())
    assert apply() == _hip.SC_OK
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(case["y"][:q])) and torch.equal(bits(e), bits(case["e"][:q]))

    idx = torch.arange(4, dtype=torch.int64, device="cuda")
    out = torch.full((q, 4), 7.0, dtype=torch.float64, device="cuda")

    def strain(coord=op._coord, n_atoms=n, dim=3, kk=k, index=idx, ks=4, rows=x, qq=q, res=out):
        return L.sc_dev_pairs_strain_f64(op.ctx.handle, p(coord), n_atoms, dim, p(op._pairs), kk, p(op._gamma), None,
                                         p(index), ks, p(rows), qq, p(res))

    assert strain(dim=2) == bad and strain(coord=None) == bad and strain(n_atoms=0) == bad
    assert strain(kk=-1) == bad and strain(qq=-1) == bad and strain(ks=-1) == bad
    assert strain(index=None) == bad and strain(res=None) == bad and strain(rows=None) == bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert strain(ks=0, index=None) == _hip.SC_OK and strain(qq=0, rows=None) == _hip.SC_OK
    assert strain() == _hip.SC_OK
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(op.strain(x, np.arange(4))))


# ---- model level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", [False, True], ids=["plain", "mass"])
@pytest.mark.parametrize("kind", ["anm", "gnm"])
def test_model_deformation_energy_and_spring_strain(sc, kind, masses):
    coord, ff = structure(sc, "n40")
    n, dim = len(coord), 3 if kind == "anm" else 1
    mass = masses_of(n) if masses else None
    atoms = coord
    if mass is not None:   # (a mass array needs an atom container, as in the reference)
        atoms = sc.AtomArray(n)
        atoms.coord = coord
    model = (sc.ANM if kind == "anm" else sc.GNM)(atoms, ff, masses=mass)
    w, v = model.eigen()
    ntriv = 6 if kind == "anm" else 1
    pairs, gamma = network(sc, coord, ff)
    scale = None if mass is None else 1.0 / np.sqrt(mass)
    h = model.hessian if kind == "anm" else model.kirchhoff

    for subset in (None, [ntriv, ntriv + 3, dim * n - 1]):
        sel = np.arange(ntriv, dim * n) if subset is None else np.array(subset)
        ref = restate(coord, pairs, gamma, scale, np.ascontiguousarray(v[sel]), dim)
        energy = model.deformation_energy(subset)
        assert isinstance(energy, np.ndarray) and energy.shape == (len(sel), n)
        assert np.all(np.abs(energy - ref["E"]) <= 1e-12 * ref["C"])
        # |v^T H v - w v^T v| <= |H v - w v| |v| (NumPy on the model's own matrix), plus the bound of the sums
        resid = np.linalg.norm(v[sel] @ h.T - w[sel, None] * v[sel], axis=1) * np.linalg.norm(v[sel], axis=1)
        gate = resid + 1e-12 * ref["C"].sum(axis=1)
        print(f"{kind} sum E - w: max {np.abs(energy.sum(axis=1) - w[sel]).max():.3e}, gate min {gate.min():.3e}")
        assert np.all(np.abs(energy.sum(axis=1) - w[sel]) <= gate)
        springs, strain = model.spring_strain(subset)
        rows = np.nonzero(pairs[:, 0] < pairs[:, 1])[0]
        assert np.array_equal(springs, pairs[rows]) and isinstance(strain, np.ndarray)
        assert strain.shape == (len(sel), len(rows))
        assert np.all(np.abs(strain - ref["S"][:, rows]) <= 1e-12 * ref["Sb"][:, rows])
        assert np.all(np.abs(strain.sum(axis=1) - w[sel]) <= gate)
    with pytest.raises(ValueError, match="Trivial"):
        model.deformation_energy([0])
    with pytest.raises(ValueError, match="Trivial"):
        sc.nma.spring_strain(model, [ntriv - 1])
    with pytest.raises(ValueError, match="GNM/ANM"):
        sc.nma.deformation_energy(object())


# ---- RTB ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", [False, True], ids=["plain", "mass"])
def test_rtb_residuals_bound_the_distance_to_the_dense_spectrum(sc, torch, masses):
    n = 60
    coord, ff = chain(n, 6), sc.InvariantForceField(10.0)
    mass = masses_of(n) if masses else None
    solver = sc.RTB(coord, ff, sc.blocks_of_consecutive(n, 3), masses=mass)
    solver.solve()
    w, v = (t[0].cpu().numpy() for t in solver.finish())
    h = sc.compute_hessian(coord, ff)[0]
    scale = None if mass is None else 1.0 / np.sqrt(mass)
    if scale is not None:
        s3 = np.repeat(scale, 3)
        h = h * np.outer(s3, s3)
    pairs, gamma = network(sc, coord, ff)
    ref = restate(coord, pairs, gamma, scale, v, 3)
    assert solver.operator is solver.operator and solver.operator._pairs.data_ptr() == solver._pairs.data_ptr()

    res = solver.residuals().cpu().numpy()
    assert res.shape == (solver.nvec,) == (len(w),)
    dense = np.linalg.norm(v @ h.T - w[:, None] * v, axis=1)
    # operator and dense product each within 1e-12 B per element of Y; w v rounds once per element
    tol = 2e-12 * np.sqrt(3 * (ref["B"] ** 2).sum(axis=1)) + 4 * np.finfo(float).eps * np.abs(w)
    print(f"rtb residuals: {res[6:].min():.3e} .. {res.max():.3e}; vs dense max err / tol {np.max(np.abs(res - dense) / tol):.3e}")
    assert np.all(np.abs(res - dense) <= tol)

    lam = np.linalg.eigvalsh(h)
    gap = np.abs(lam[None, :] - w[6:, None]).min(axis=1)
    assert np.all(gap <= res[6:] + 1e-10 * lam.max())
    assert np.all(res[:6] <= 1e-10 * lam.max())   # (rigid-body motions lie in the block space)

    energy = solver.deformation_energy()
    assert energy.shape == (solver.nvec - 6, n) and energy.is_cuda
    energy = energy.cpu().numpy()
    assert np.all(np.abs(energy - ref["E"][6:]) <= 1e-12 * ref["C"][6:])
    # |v^T H v - w| <= residual for a unit v; the modes are unit vectors to 1e-12 (the RTB tests' gate)
    gate = res[6:] + 1e-12 * ref["C"][6:].sum(axis=1) + 1e-12 * np.abs(w[6:])
    assert np.all(np.abs(energy.sum(axis=1) - w[6:]) <= gate)

    springs, strain = solver.spring_strain([6, 9, 20])
    rows = np.nonzero(pairs[:, 0] < pairs[:, 1])[0]
    assert np.array_equal(springs, pairs[rows]) and strain.shape == (3, len(rows))
    assert np.all(np.abs(strain.cpu().numpy() - ref["S"][[6, 9, 20]][:, rows]) <= 1e-12 * ref["Sb"][[6, 9, 20]][:, rows])
    assert np.allclose(solver.residuals([6, 9, 20]).cpu().numpy(), res[[6, 9, 20]], rtol=1e-13, atol=0)
    assert torch.equal(bits(solver.deformation_energy([9])[0]), bits(solver.deformation_energy()[3]))
    with pytest.raises(ValueError, match="Trivial"):
        solver.deformation_energy([2])

    # a partial solve: rows are modes lo .. hi
    solver.solve(subset_by_index=(4, 15))
    solver.finish()
    part = solver.residuals().cpu().numpy()
    w_part = solver.w[0].cpu().numpy()
    assert part.shape == (12,)
    assert np.all(np.abs(lam[None, :] - w_part[2:, None]).min(axis=1) <= part[2:] + 1e-10 * lam.max())
    assert solver.deformation_energy().shape == (10, n)
    assert solver.spring_strain([7])[1].shape == (1, len(rows))
