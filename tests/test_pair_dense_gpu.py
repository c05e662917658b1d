"""
GPU tests of the pair-list kernels on atoms with 63 .. 130 pairs: ``pair_walk`` of csrc/pair_walk.h inside ``k_pairs_panel``
(``PairOperator.panel_step``, ``sc_dev_pairs_panel_f64``) and ``k_cg_apply_dot`` (``sc_dev_pairs_cg_step_f64``), and
``k_pairs_apply`` (csrc/pair_operator.hip).  All three take an atom's pairs 64 at a time; the jittered lattices under a 7 A
cutoff of the other pair-list tests give an atom at most 26 pairs, one partly filled chunk.  Here every atom reaches

    a full chunk             (64 pairs: the all-ones mask of the listed lanes, the four-pair loop run to its end),
    every chunk after the first   (the reload of the lanes' pairs, the carry of the sums), and
    the skipped-row path     (a row whose first atom is not the wavefront's or whose second lies outside 0 .. N - 1).

Networks (tests/test_pair_dense_host.py, which asserts the pair counts without a GPU): the dense lattices D64, D65, D66, D129,
D131 under ``HinsenForceField()`` with 63, 64, 65, 128, 130 pairs per atom; MIX, D66 without three springs through
``PairOperator.from_pairs`` (64, 64, 63, 64 | 64, 65, 65, 65 pairs in the first two workgroups, so the wavefronts of a
workgroup make different numbers of trips before the barrier of ``k_cg_apply_dot``); the unchecked lists U1 and U2 for the C
entries.  Each in dim 3 and dim 1, with and without masses ``RandomState(5).uniform(50, 200, N)``, unless a test says
otherwise.  N = 65, 66, 129, 131 leave a ragged last workgroup of four atoms.  Panels: 65 ``RandomState(21).standard_normal``
columns, q in {1, 64, 65}, ld in {q, q + 3}.

References and gates are those of the files the helpers come from: the NumPy restatement (:func:`restate`) within
``|alpha| 1e-12 t_i B_i + 4 eps (|beta| |X| + |gamma_c| |Z0|)`` -- derived for sums of fewer than 1000 terms per atom; 130 pairs
of three components are 390 -- the dense NumPy matrix within the same, equal bits where the kernels promise them, the dots
within ``m 2^-52 sum |terms|``, one CG iteration within ``1e-13 (|value| + b |P|_max)``.

The unchecked lists cannot make a correct kernel read outside its arguments; so that a kernel whose guard were broken
would not either, they use only the atoms -1 and N, and the coordinates, the atom scale and every panel are views inside
larger tensors with at least one atom's rows of NaN on each side: a row that is not skipped shows as NaN or as a wrong
number, and the margins are compared afterwards.  Each unchecked case runs each entry once.

End to end on D131 (plain and mass-weighted) and on D66 as a GNM, ``tol = 1e-10``.  The caps are conditions, not
measurements: the NumPy prototypes of the drivers need 148, 184 and 38 CG iterations (cap 600) and 11 and 18 filter passes for
``lowest_modes(12)`` at degree 20 (cap 60), a third of the cap at most (tests/test_pair_dense_host.py asserts it).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from springcraft_amd import iterative
from tests.test_iterative_host import masses_of, np_matrix
from tests.test_pair_cg_gpu import Run
from tests.test_pair_dense_host import (DEGREE, DENSE, K_MODES, MIX_COUNTS, MODES_MAX_ITER, SOLVE_MAX_ITER, TOL, dense_network,
                                        unchecked)
from tests.test_pair_operator_gpu import bits, network, restate
from tests.test_pair_panel_gpu import COEFS, SENTINEL, panel_reference, run
from tests.test_solve_host import check_solution, right_hand_sides

pytestmark = pytest.mark.gpu

QS = (1, 64, 65)
QMAX = 65
EPS = np.finfo(float).eps
MARGIN = 3   # rows of NaN on each side of an embedded buffer: one atom's worth
_cache = {}


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def grid(names, dims=(3, 1)):
    keys = [(name, masses, dim) for name in names for dim in dims for masses in (False, True)]
    return {"argnames": "key", "argvalues": keys,
            "ids": [f"{name}-dim{dim}-{'mass' if masses else 'plain'}" for name, masses, dim in keys]}


def case_of(sc, torch, key):
    """A network's operator, 65 columns, their restatement and the dense NumPy matrix, built once per (name, masses, dim)."""
    if key not in _cache:
        name, masses, dim = key
        coord, pairs, gamma = dense_network(name)
        n = len(coord)
        mass = masses_of(n) if masses else None
        scale = None if mass is None else 1.0 / np.sqrt(mass)
        if name == "MIX":
            op = sc.PairOperator.from_pairs(coord, pairs, gamma, dim=dim, inv_sqrt_mass=scale)
            assert list(np.bincount(op.pairs[:, 0], minlength=n)[:8]) == MIX_COUNTS
        else:   # the package's own list and constants: the rows the host file writes down
            ff = sc.HinsenForceField()
            op = sc.PairOperator(coord, ff, dim=dim, masses=mass)
            listed, gamma = network(sc, coord, ff)
            assert np.array_equal(listed, pairs) and np.array_equal(op.pairs, pairs)
            assert np.allclose(op.gamma, gamma, rtol=1e-14, atol=0)
            assert np.array_equal(np.bincount(op.pairs[:, 0], minlength=n), np.full(n, DENSE[name][1] - 1))
        rng = np.random.RandomState(21)
        x, z0 = rng.standard_normal((dim * n, QMAX)), rng.standard_normal((dim * n, QMAX))
        hx, tb = panel_reference(coord, pairs, gamma, scale, x, dim)
        xd = torch.from_numpy(x).cuda()
        _cache[key] = {"name": name, "coord": coord, "pairs": pairs, "gamma": gamma, "scale": scale, "mass": mass, "n": n,
                       "dim": dim, "m": dim * n, "op": op, "x": x, "z0": z0, "hx": hx, "tb": tb, "xd": xd, "fd": xd, "f": x,
                       "zd": torch.from_numpy(z0).cuda(), "h": np_matrix(coord, pairs, gamma, dim, scale),
                       "b": op.spectral_bound()}
    return _cache[key]


def panel_gate(alpha, beta, gamma_c, tb, x, z0):
    return abs(alpha) * 1e-12 * tb + 4 * EPS * (abs(beta) * np.abs(x) + abs(gamma_c) * np.abs(z0))


def ratio(err, tol):
    return float(np.max(err / np.where(tol > 0, tol, 1)))


# ---- 1: the panel step against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize(**grid(("D64", "D65", "D66", "D129", "D131", "MIX")))
def test_panel_step_matches_the_restatement_and_leaves_the_padding(sc, torch, key):
    case = case_of(sc, torch, key)
    worst = 0.0
    for q in QS:
        for ld in (q, q + 3):
            for alpha, beta, gamma_c in COEFS:
                z = run(torch, case, q, ld, (alpha, beta, gamma_c)).cpu().numpy()
                x, z0 = case["x"][:, :q], case["z0"][:, :q]
                ref = alpha * case["hx"][:, :q] + beta * x + gamma_c * z0
                tol = panel_gate(alpha, beta, gamma_c, case["tb"][:, :q], x, z0)
                err = np.abs(z[:, :q] - ref)
                worst = max(worst, ratio(err, tol))
                assert np.all(err <= tol), (q, ld, alpha)
                assert np.all(z[:, q:] == SENTINEL), (q, ld, alpha)   # columns q .. ld - 1 keep their bits
    print(f"panel vs restatement: max err / tol {worst:.3e}")


# ---- 2: the panel step against apply and the dense matrix ----------------------------------------------------------------
@pytest.mark.parametrize(**grid(("D65", "D131")))
def test_panel_step_matches_apply_and_the_dense_matrix(sc, torch, key):
    case = case_of(sc, torch, key)
    z = run(torch, case, QMAX, QMAX, COEFS[0])
    y = case["op"].apply(case["xd"].T.contiguous()).T
    tol = 1e-12 * case["tb"]
    err_apply = (z - y).abs().cpu().numpy()
    err_dense = np.abs(z.cpu().numpy() - case["h"] @ case["x"])
    print(f"panel vs apply: max err / tol {ratio(err_apply, tol):.3e}; vs dense matrix: {ratio(err_dense, tol):.3e}")
    assert np.all(err_apply <= tol) and np.all(err_dense <= tol)


# ---- 3: bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**grid(("D66", "D131")))
def test_a_column_has_the_same_bits_alone_and_a_nan_column_stays_alone(sc, torch, key):
    case = case_of(sc, torch, key)
    for coef in COEFS:
        full = run(torch, case, QMAX, QMAX, coef)
        assert torch.equal(bits(run(torch, case, QMAX, QMAX, coef)), bits(full))   # two calls
        for r in (0, 63, 64):
            one = slice(r, r + 1)
            for ld in (1, 4):
                alone = run(torch, case, 1, ld, coef, x=case["xd"][:, one], z0=case["zd"][:, one])
                assert torch.equal(bits(alone[:, 0]), bits(full[:, r])), (r, ld)
    clean = run(torch, case, QMAX, QMAX, COEFS[1])
    for r in (0, 64):
        bad = case["xd"].clone()
        bad[:, r] = float("nan")
        z = run(torch, case, QMAX, QMAX, COEFS[1], x=bad)
        keep = [c for c in range(QMAX) if c != r]
        assert torch.equal(bits(z[:, keep]), bits(clean[:, keep]))
        assert bool(torch.isnan(z[:, r]).all())   # (every atom has pairs)


# ---- 4: CG, Q and the dots -----------------------------------------------------------------------------------------------
def dots_ratio(run_, f, m):
    """``|pq - sum| / bound`` and ``|rho - sum| / bound`` of a run after its first iteration, per column."""
    q = run_.q
    Q, R = (t[:, :q].cpu().numpy() for t in (run_.Q, run_.R))
    t_pq, t_rr = f[:, :q] * Q, R * R
    e_pq = np.abs(run_.row("pq") - t_pq.sum(axis=0)) / (m * 2.0 ** -52 * np.abs(t_pq).sum(axis=0))
    e_rr = np.abs(run_.row("rho") - t_rr.sum(axis=0)) / (m * 2.0 ** -52 * t_rr.sum(axis=0))
    return e_pq, e_rr


@pytest.mark.parametrize(**grid(("D65", "D66", "D131", "MIX")))
def test_cg_q_has_the_bits_of_the_panel_step_and_the_dots_are_its_sums(sc, torch, key):
    case = case_of(sc, torch, key)
    worst = 0.0
    for q in (1, QMAX):
        for ld in (q, q + 3):
            cg = Run(torch, case, slice(0, q), ld).init().step()
            z = torch.empty((case["m"], q), dtype=torch.float64, device="cuda")
            case["op"].panel_step(case["fd"][:, :q].contiguous(), z, 1.0, 0.0, 0.0)
            assert torch.equal(bits(cg.Q[:, :q]), bits(z)), (q, ld)
            assert cg.padding_is_untouched(), (q, ld)
            e_pq, e_rr = dots_ratio(cg, case["f"], case["m"])
            worst = max(worst, float(e_pq.max()), float(e_rr.max()))
            assert np.all(e_pq <= 1) and np.all(e_rr <= 1), (q, ld)
            assert np.all(cg.row("iters") == 1) and np.all(cg.row("status") == 0)
    print(f"dots: max |device - sum| / bound {worst:.3f}")


# ---- 5: CG, one iteration ------------------------------------------------------------------------------------------------
def recurrence_ratio(h, b, f, X, R, P):
    """The worst ``err / gate`` of X, R, P after one iteration against the NumPy recurrence on the dense matrix ``h``."""
    q_ref = h @ f
    rho0 = (f * f).sum(axis=0)
    alpha = rho0 / (f * q_ref).sum(axis=0)
    x_ref, r_ref = alpha * f, f - alpha * q_ref
    p_ref = r_ref + ((r_ref * r_ref).sum(axis=0) / rho0) * f
    worst = {}
    for name, got, ref in (("X", X, x_ref), ("R", R, r_ref), ("P", P, p_ref)):
        gate = 1e-13 * (np.abs(ref) + b * np.abs(f).max())
        worst[name] = float((np.abs(got - ref) / gate).max())
    return worst


@pytest.mark.parametrize(**grid(("D66", "D131", "MIX")))
def test_cg_iteration_matches_the_numpy_recurrence_and_a_column_alone(sc, torch, key):
    case = case_of(sc, torch, key)
    cg = Run(torch, case, slice(0, QMAX), QMAX + 3).init()
    rho0 = cg.row("rho")
    cg.step()
    X, R, P = (t[:, :QMAX].cpu().numpy() for t in (cg.X, cg.R, cg.P))
    assert np.array_equal(cg.row("alpha"), rho0 / cg.row("pq")) and np.array_equal(cg.row("beta"), cg.row("rho") / rho0)
    worst = recurrence_ratio(case["h"], case["b"], case["f"], X, R, P)
    print(f"one iteration vs NumPy: max err / gate {max(worst.values()):.3e}")
    assert all(v <= 1 for v in worst.values()), worst
    assert cg.padding_is_untouched()
    # alone and in the batch, two iterations
    full = Run(torch, case, slice(0, QMAX)).init().step(2)
    for c in (0, 63, 64):
        for ld in (1, 4):
            alone = Run(torch, case, slice(c, c + 1), ld).init().step(2)
            assert torch.equal(alone.column_bits(0), full.column_bits(c)), (c, ld)
            assert alone.padding_is_untouched()


# ---- 6: unchecked lists through the C entries ----------------------------------------------------------------------------
def embedded(torch, data, margin=MARGIN):
    """``data`` (rows, cols) as a view in the middle of a NaN tensor with ``margin`` more rows on each side: (buffer, view)."""
    rows = data.shape[0]
    buf = torch.full((rows + 2 * margin,) + tuple(data.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[margin: margin + rows]
    view.copy_(data)
    return buf, view


def margins_are_nan(torch, buf, margin=MARGIN):
    return bool(torch.isnan(buf[:margin]).all()) and bool(torch.isnan(buf[len(buf) - margin:]).all())


class EmbeddedRun(Run):
    """A CG run whose four panels lie between NaN margins."""

    def __init__(self, torch, case, cols, ld):
        super().__init__(torch, case, cols, ld)
        self.buffers = {}
        for name in ("X", "R", "P", "Q"):
            self.buffers[name], view = embedded(torch, getattr(self, name))
            setattr(self, name, view)


def unchecked_case(sc, torch, key):
    if key not in _cache:
        name, masses, dim = key
        base = case_of(sc, torch, ("D66", masses, dim))
        coord, pairs, gamma, start, keep = unchecked(name)
        n, scale = base["n"], base["scale"]
        clean_pairs, clean_gamma = pairs[keep], gamma[keep]
        hx, tb = panel_reference(coord, clean_pairs, clean_gamma, scale, base["x"], dim)
        raw = SimpleNamespace(ctx=base["op"].ctx, n_atoms=n, dim=dim, n_pairs=len(pairs))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        raw.coord_buf, raw._coord = embedded(torch, dev(coord))
        raw.scale_buf, raw._scale = (None, None) if scale is None else embedded(torch, dev(scale))
        raw._pairs, raw._gamma, raw._row_start = dev(pairs), dev(gamma), dev(start)
        _cache[key] = dict(base, name=name, op=raw, pairs=pairs, keep=keep, clean=(clean_pairs, clean_gamma), hx=hx, tb=tb,
                           h=np_matrix(coord, clean_pairs, clean_gamma, dim, scale),
                           b=iterative.spectral_bound(clean_pairs, clean_gamma, n, scale))
    return _cache[key]


def inputs_are_intact(torch, case):
    raw = case["op"]
    ok = margins_are_nan(torch, raw.coord_buf) and np.array_equal(raw._coord.cpu().numpy(), case["coord"])
    if raw._scale is not None:
        ok = ok and margins_are_nan(torch, raw.scale_buf) and np.array_equal(raw._scale.cpu().numpy(), case["scale"])
    return ok


def skipped_rows(case):
    """The matrix rows of atom 7, all of whose pairs U2 skips."""
    return slice(case["dim"] * 7, case["dim"] * 8)


@pytest.mark.parametrize(**grid(("U1", "U2")))
def test_unchecked_rows_are_skipped_by_the_panel_step(sc, torch, key):
    from springcraft_amd import _hip

    case = unchecked_case(sc, torch, key)
    raw, m, q, ld = case["op"], case["m"], QMAX, QMAX + 3
    alpha, beta, gamma_c = COEFS[1]
    pad = lambda t: torch.cat([t, torch.full((m, ld - q), SENTINEL, dtype=torch.float64, device="cuda")], dim=1)   # noqa: E731
    xbuf, xv = embedded(torch, pad(case["xd"]))
    zbuf, zv = embedded(torch, pad(case["zd"]))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    status = _hip.lib().sc_dev_pairs_panel_f64(raw.ctx.handle, p(raw._coord), raw.n_atoms, raw.dim, p(raw._pairs), raw.n_pairs,
                                               p(raw._gamma), p(raw._row_start), p(raw._scale), p(xv), p(zv), ld, q, alpha, beta,
                                               gamma_c)
    assert status == _hip.SC_OK
    torch.cuda.synchronize()
    z = zv.cpu().numpy()
    x, z0 = case["x"], case["z0"]
    ref = alpha * case["hx"] + beta * x + gamma_c * z0
    tol = panel_gate(alpha, beta, gamma_c, case["tb"], x, z0)
    assert np.all(np.isfinite(z[:, :q]))
    err = np.abs(z[:, :q] - ref)
    print(f"{case['name']} panel vs the restatement of the cleaned list: max err / tol {ratio(err, tol):.3e}")
    assert np.all(err <= tol)
    assert np.all(z[:, q:] == SENTINEL) and torch.equal(bits(xv), bits(pad(case["xd"])))
    assert margins_are_nan(torch, xbuf) and margins_are_nan(torch, zbuf) and inputs_are_intact(torch, case)
    if case["name"] == "U2":
        rows = skipped_rows(case)
        assert np.array_equal(z[rows, :q], beta * x[rows] + gamma_c * z0[rows])


@pytest.mark.parametrize(**grid(("U1", "U2")))
def test_unchecked_rows_are_skipped_by_apply_and_energy(sc, torch, key):
    from springcraft_amd import _hip

    case = unchecked_case(sc, torch, key)
    raw, n, dim, m, q = case["op"], case["n"], case["dim"], case["m"], 4
    rows = np.ascontiguousarray(case["x"][:, :q].T)
    ref = restate(case["coord"], *case["clean"], case["scale"], rows, dim)
    xbuf, xv = embedded(torch, torch.from_numpy(rows).cuda(), margin=1)   # (a margin of one row of m >= 3 doubles)
    ybuf, yv = embedded(torch, torch.full((q, m), SENTINEL, dtype=torch.float64, device="cuda"), margin=1)
    ebuf, ev = embedded(torch, torch.full((q, n), SENTINEL, dtype=torch.float64, device="cuda"), margin=1)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    status = _hip.lib().sc_dev_pairs_apply_f64(raw.ctx.handle, p(raw._coord), n, dim, p(raw._pairs), raw.n_pairs, p(raw._gamma),
                                               p(raw._row_start), p(raw._scale), p(xv), q, p(yv), p(ev))
    assert status == _hip.SC_OK
    torch.cuda.synchronize()
    y, e = yv.cpu().numpy(), ev.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(e))
    err_y, tol_y = np.abs(y - ref["Y"]), 1e-12 * np.repeat(ref["B"], dim, axis=1)
    err_e, tol_e = np.abs(e - ref["E"]), 1e-12 * ref["C"]
    print(f"{case['name']} apply vs the restatement of the cleaned list: Y max err / tol {ratio(err_y, tol_y):.3e}, "
          f"E {ratio(err_e, tol_e):.3e}")
    assert np.all(err_y <= tol_y) and np.all(err_e <= tol_e) and np.all(e >= 0)
    assert all(margins_are_nan(torch, b, 1) for b in (xbuf, ybuf, ebuf)) and inputs_are_intact(torch, case)
    assert np.array_equal(xv.cpu().numpy(), rows)
    if case["name"] == "U2":
        assert np.all(y[:, skipped_rows(case)] == 0.0) and np.all(e[:, 7] == 0.0)


@pytest.mark.parametrize(**grid(("U1", "U2")))
def test_unchecked_rows_are_skipped_by_a_cg_iteration(sc, torch, key):
    case = unchecked_case(sc, torch, key)
    cg = EmbeddedRun(torch, case, slice(0, QMAX), QMAX + 3).init().step()
    torch.cuda.synchronize()
    X, R, P, Q = (t[:, :QMAX].cpu().numpy() for t in (cg.X, cg.R, cg.P, cg.Q))
    assert all(np.all(np.isfinite(t)) for t in (X, R, P, Q))
    assert all(np.all(np.isfinite(cg.row(k))) for k in ("rho", "pq", "alpha", "beta"))
    assert np.all(cg.row("iters") == 1) and np.all(cg.row("status") == 0)
    err, tol = np.abs(Q - case["hx"]), 1e-12 * case["tb"]
    e_pq, e_rr = dots_ratio(cg, case["f"], case["m"])
    worst = recurrence_ratio(case["h"], case["b"], case["f"], X, R, P)
    print(f"{case['name']} CG: Q vs the restatement of the cleaned list max err / tol {ratio(err, tol):.3e}; dots / bound "
          f"{max(e_pq.max(), e_rr.max()):.3f}; one iteration vs NumPy max err / gate {max(worst.values()):.3e}")
    assert np.all(err <= tol)
    assert np.all(e_pq <= 1) and np.all(e_rr <= 1)
    assert all(v <= 1 for v in worst.values()), worst
    assert cg.padding_is_untouched()
    assert all(margins_are_nan(torch, b) for b in cg.buffers.values()) and inputs_are_intact(torch, case)
    if case["name"] == "U2":
        assert np.all(Q[skipped_rows(case)] == 0.0)


def test_from_pairs_refuses_an_unchecked_list_on_the_host(sc, torch):
    for name in ("U1", "U2"):
        coord, pairs, gamma, _, _ = unchecked(name)
        for dim in (3, 1):
            with pytest.raises(ValueError, match="outside"):
                sc.PairOperator.from_pairs(coord, pairs, gamma, dim=dim)


# ---- 7: k_pairs_apply at exactly 64 and 128 pairs ------------------------------------------------------------------------
@pytest.mark.parametrize(**grid(("D65", "D129"), dims=(3,)))
def test_apply_and_energy_at_full_chunks(sc, torch, key):
    case = case_of(sc, torch, key)
    op, dim = case["op"], case["dim"]
    x = np.random.RandomState(11).standard_normal((9, case["m"]))
    xd = torch.from_numpy(x).cuda()
    ref = restate(case["coord"], case["pairs"], case["gamma"], case["scale"], x, dim)
    y, e = op.apply_energy(xd)
    err_y, tol_y = np.abs(y.cpu().numpy() - ref["Y"]), 1e-12 * np.repeat(ref["B"], dim, axis=1)
    err_e, tol_e = np.abs(e.cpu().numpy() - ref["E"]), 1e-12 * ref["C"]
    print(f"Y: max err / tol {ratio(err_y, tol_y):.3e}; E: {ratio(err_e, tol_e):.3e}")
    assert np.all(err_y <= tol_y) and np.all(err_e <= tol_e) and bool((e >= 0).all())
    for q in (1, 4, 5):   # a row's bits do not depend on how many rows there are, nor on its position
        yq, eq = op.apply_energy(xd[:q])
        assert torch.equal(bits(yq), bits(y[:q])) and torch.equal(bits(eq), bits(e[:q]))
    for r in (0, 3, 8):
        y1, e1 = op.apply_energy(xd[r: r + 1])
        assert torch.equal(bits(y1[0]), bits(y[r])) and torch.equal(bits(e1[0]), bits(e[r]))
    assert torch.equal(bits(op.apply(xd)), bits(y)) and torch.equal(bits(op.energy(xd)), bits(e))


# ---- 8: end to end -------------------------------------------------------------------------------------------------------
def package_matrix(sc, case):
    dim = case["dim"]
    h = (sc.compute_hessian if dim == 3 else sc.compute_kirchhoff)(case["coord"], sc.HinsenForceField())[0]
    if case["scale"] is not None:
        s = np.repeat(case["scale"], dim)
        h = h * np.outer(s, s)
    return h


@pytest.mark.parametrize(**grid(("D131",), dims=(3,)))
def test_lowest_modes_of_a_dense_network_are_the_dense_eigenpairs(sc, torch, key):
    case = case_of(sc, torch, key)
    k, h = K_MODES, package_matrix(sc, case)
    lam = np.linalg.eigvalsh(h)
    w, v, info = case["op"].lowest_modes(k, tol=TOL, degree=DEGREE, max_iter=MODES_MAX_ITER, seed=0)
    assert tuple(w.shape) == (k,) and tuple(v.shape) == (k, len(h))
    w, v = w.cpu().numpy(), v.cpu().numpy()
    b = info["b"]
    res = np.linalg.norm(v @ h.T - w[:, None] * v, axis=1)
    print(f"{info['iterations']} passes (cap {MODES_MAX_ITER}), {info['panel_steps']} panel steps; b = {b:.6g}, lambda_max = "
          f"{lam[-1]:.6g}; max |w - lambda| / b {np.abs(w - lam[:k]).max() / b:.2e}, max residual / b {res.max() / b:.2e}, "
          f"|V V^T - I| {np.abs(v @ v.T - np.eye(k)).max():.2e}")
    assert info["converged"] and info["iterations"] <= MODES_MAX_ITER
    assert info["panel_steps"] == info["iterations"] * (DEGREE + 1) + 1
    assert b == case["op"].spectral_bound() and b >= lam[-1]
    gate = TOL * b + 1e-12 * b
    assert np.all(np.diff(w) >= 0)
    assert np.all(np.abs(w - lam[:k]) <= gate)
    assert np.all(res <= gate) and np.all(info["residuals"] <= TOL * b)
    assert np.abs(v @ v.T - np.eye(k)).max() <= 1e-12


@pytest.mark.parametrize("key", [("D131", False, 3), ("D131", True, 3), ("D66", False, 1)],
                         ids=["D131-plain", "D131-mass", "D66-gnm"])
def test_solve_on_a_dense_network_is_the_dense_pseudo_inverse(sc, torch, key):
    case = case_of(sc, torch, key)
    op, h = case["op"], package_matrix(sc, case)
    f = right_hand_sides(case["n"], case["dim"])
    x, info = op.solve(f, tol=TOL, max_iter=SOLVE_MAX_ITER)
    assert x.is_cuda and tuple(x.shape) == f.shape and info["b"] == case["b"] and info["tol"] == TOL
    check_solution(x.cpu().numpy(), info, h, op.null_space().cpu().numpy(), case["b"], f, tol=TOL,
                   label=f"{case['name']} dim {case['dim']}, device (cap {SOLVE_MAX_ITER})")
    assert info["converged"] and info["iterations"].max() <= SOLVE_MAX_ITER
