"""
GPU tests of one conjugate-gradient iteration through the C entries ``sc_dev_pairs_cg_workspace``,
``sc_dev_pairs_cg_init_f64`` and ``sc_dev_pairs_cg_step_f64`` (csrc/pair_cg.hip).

Structures (tests/test_solve_host.py): A = ``lattice(4, 5, 6, 3)`` (N = 120, 30 full workgroups) and A19, A without its last
atom (N = 119: the last workgroup has three atoms), under ``InvariantForceField(7.0)``, in dim 3 and dim 1, with and without
masses ``RandomState(5).uniform(50, 200, N)``; the operator tests' ``chain(40, 2)`` with atom 17 moved away for an atom
without pairs.  Panels: q in {1, 64, 65} (65 crosses a chunk of 64 columns), ld in {q, q + 3}, the padding and every
untouched word prefilled with a sentinel.  The right-hand sides are 65 ``RandomState(21).standard_normal`` columns.

References and gates.  ``Q`` must have the bits of ``panel_step(P, Q, 1, 0, 0)``.  The reduced dots ``pq`` and ``rho`` lie within
``m 2^-52 sum |terms|`` of NumPy's sums of the device's own ``P Q`` and ``R R``, the bound of any summation order.  After one
iteration ``X``, ``R``, ``P`` are compared with the NumPy recurrence on the dense matrix within ``1e-13 (|value| + b |P|_max)``
elementwise: a few roundings of a product with a matrix of norm at most b.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_iterative_host import masses_of, np_matrix
from tests.test_pair_operator_gpu import ISOLATED, bits, structure
from tests.test_solve_host import coord_of

pytestmark = pytest.mark.gpu

QS = (1, 64, 65)
QMAX = 65
SENTINEL = -7.25
TOL = 1e-10
ROWS = {"rho": 0, "stop": 1, "alpha": 2, "beta": 3, "status": 4, "iters": 5, "pq": 6}
CASES = [(name, masses, dim) for name in ("A", "A19") for dim in (3, 1) for masses in (False, True)]
CASE_IDS = [f"{name}-dim{dim}-{'mass' if masses else 'plain'}" for name, masses, dim in CASES]
_cache = {}


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def case_of(sc, torch, key):
    if key not in _cache:
        name, masses, dim = key
        coord, ff = (structure(sc, name) if name == "n40iso" else (coord_of(name), sc.InvariantForceField(7.0)))
        n = len(coord)
        mass = masses_of(n) if masses else None
        op = sc.PairOperator(coord, ff, dim=dim, masses=mass)
        if name == "n40iso":   # the same list through from_pairs
            op = sc.PairOperator.from_pairs(coord, op.pairs, op.gamma, dim=dim)
        scale = None if mass is None else 1.0 / np.sqrt(mass)
        f = np.random.RandomState(21).standard_normal((dim * n, QMAX))
        _cache[key] = {"op": op, "n": n, "dim": dim, "m": dim * n, "f": f, "fd": torch.from_numpy(f).cuda(),
                       "h": np_matrix(coord, op.pairs, op.gamma, dim, scale), "b": op.spectral_bound()}
    return _cache[key]


@pytest.fixture(params=CASES, ids=CASE_IDS)
def case(request, sc, torch):
    return case_of(sc, torch, request.param)


class Run:
    """Panels and state of one solve inside sentinel-filled buffers of leading dimension ld."""

    def __init__(self, torch, case, cols, ld=None, rhs=None):
        from springcraft_amd import _hip

        self.torch, self.op, self.L = torch, case["op"], _hip.lib()
        f = (case["fd"] if rhs is None else rhs)[:, cols]
        self.q, self.m = f.shape[1], case["m"]
        self.ld = self.q if ld is None else ld
        full = lambda rows: torch.full((rows, self.ld), SENTINEL, dtype=torch.float64, device="cuda")   # noqa: E731
        self.X, self.R, self.P, self.Q, self.state = full(self.m), full(self.m), full(self.m), full(self.m), full(7)
        self.R[:, : self.q] = f
        size = C.c_size_t()
        assert self.L.sc_dev_pairs_cg_workspace(self.op.n_atoms, self.q, C.byref(size)) == _hip.SC_OK
        assert size.value == 8 * self.q * ((self.op.n_atoms + 3) // 4)
        self.bytes = size.value
        self.work = torch.full((size.value // 8 + 5,), SENTINEL, dtype=torch.float64, device="cuda")
        self.p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def init(self, tol=TOL):
        op, p = self.op, self.p
        op.ctx.check(self.L.sc_dev_pairs_cg_init_f64(op.ctx.handle, op.n_atoms, op.dim, p(self.X), p(self.R), p(self.P),
                                                     self.ld, self.q, tol, p(self.state), p(self.work), self.bytes))
        return self

    def step(self, iterations=1):
        op, p = self.op, self.p
        have = op.n_pairs > 0
        op.ctx.check(self.L.sc_dev_pairs_cg_step_f64(
            op.ctx.handle, p(op._coord), op.n_atoms, op.dim, p(op._pairs) if have else None, op.n_pairs,
            p(op._gamma) if have else None, p(op._row_start), p(op._scale), p(self.X), p(self.R), p(self.P), p(self.Q),
            self.ld, self.q, p(self.state), p(self.work), self.bytes, iterations))
        return self

    def row(self, name):
        """A state row's live columns on the host."""
        r = self.state[ROWS[name], : self.q]
        return (r.view(self.torch.int64) if name in ("status", "iters") else r).cpu().numpy()

    def set_status(self, col, value):
        self.state[ROWS["status"]].view(self.torch.int64)[col] = value

    def column_bits(self, c):
        """The bits of what a column owns: X, R, P, rho, iters."""
        return self.torch.cat([bits(t[:, c]) for t in (self.X, self.R, self.P)]
                              + [bits(self.state[ROWS[k], c: c + 1]) for k in ("rho", "iters")])

    def padding_is_untouched(self):
        tail = [t[:, self.q:] for t in (self.X, self.R, self.P, self.Q, self.state)] + [self.work[self.bytes // 8:]]
        return all(bool((t == SENTINEL).all()) for t in tail)


def test_init_sets_the_start_of_a_solve(case, torch):
    for q in QS:
        for ld in (q, q + 3):
            run = Run(torch, case, slice(0, q), ld).init()
            f = case["f"][:, :q]
            assert torch.equal(bits(run.P[:, :q]), bits(case["fd"][:, :q])) and bool((run.X[:, :q] == 0).all())
            rho = run.row("rho")
            assert np.all(np.abs(rho - (f * f).sum(axis=0)) <= case["m"] * 2.0 ** -52 * (f * f).sum(axis=0))
            assert np.array_equal(run.row("stop"), TOL * TOL * rho)
            assert np.all(run.row("status") == 0) and np.all(run.row("iters") == 0)
            assert run.padding_is_untouched()


def test_q_has_the_bits_of_the_panel_step(case, torch):
    for q in QS:
        for ld in (q, q + 3):
            run = Run(torch, case, slice(0, q), ld).init().step()
            z = torch.empty((case["m"], q), dtype=torch.float64, device="cuda")
            case["op"].panel_step(case["fd"][:, :q].contiguous(), z, 1.0, 0.0, 0.0)
            assert torch.equal(bits(run.Q[:, :q]), bits(z)), (q, ld)
            assert run.padding_is_untouched(), (q, ld)


def test_one_iteration_matches_the_numpy_recurrence(case, torch):
    h, b, m, f = case["h"], case["b"], case["m"], case["f"]
    run = Run(torch, case, slice(0, QMAX), QMAX + 3).init()
    rho0 = run.row("rho")
    run.step()
    X, R, P, Q = (t[:, :QMAX].cpu().numpy() for t in (run.X, run.R, run.P, run.Q))
    # the reduced dots against NumPy's sums of the same terms
    pq, rho = run.row("pq"), run.row("rho")
    t_pq, t_rr = f * Q, R * R
    e_pq = np.abs(pq - t_pq.sum(axis=0)) / (m * 2.0 ** -52 * np.abs(t_pq).sum(axis=0))
    e_rr = np.abs(rho - t_rr.sum(axis=0)) / (m * 2.0 ** -52 * t_rr.sum(axis=0))
    print(f"dots: |pq - sum| / bound {e_pq.max():.3f}, |rho - sum| / bound {e_rr.max():.3f}")
    assert np.all(e_pq <= 1) and np.all(e_rr <= 1)
    assert np.array_equal(run.row("alpha"), rho0 / pq) and np.array_equal(run.row("beta"), rho / rho0)
    assert np.all(run.row("iters") == 1) and np.all(run.row("status") == 0)
    # the recurrence
    q_ref = h @ f
    alpha = (f * f).sum(axis=0) / (f * q_ref).sum(axis=0)
    x_ref, r_ref = alpha * f, f - alpha * q_ref
    p_ref = r_ref + ((r_ref * r_ref).sum(axis=0) / (f * f).sum(axis=0)) * f
    worst = 0.0
    for name, got, ref in (("X", X, x_ref), ("R", R, r_ref), ("P", P, p_ref)):
        gate = 1e-13 * (np.abs(ref) + b * np.abs(f).max())
        worst = max(worst, float((np.abs(got - ref) / gate).max()))
        assert np.all(np.abs(got - ref) <= gate), name
    print(f"one iteration vs NumPy: max err / gate {worst:.3e}")


def test_a_column_has_the_same_bits_alone_and_in_a_batch(case, torch):
    full = Run(torch, case, slice(0, QMAX)).init().step(2)
    again = Run(torch, case, slice(0, QMAX)).init().step(2)
    for t, u in ((full.X, again.X), (full.R, again.R), (full.P, again.P), (full.Q, again.Q), (full.state, again.state)):
        assert torch.equal(bits(t), bits(u))   # two runs
    wide = Run(torch, case, slice(0, QMAX), QMAX + 3).init().step(2)
    split = Run(torch, case, slice(0, QMAX)).init().step().step()   # one call of two iterations or two of one
    for c in (0, 63, 64):
        assert torch.equal(wide.column_bits(c), full.column_bits(c)) and torch.equal(split.column_bits(c), full.column_bits(c))
        for ld in (1, 4):
            alone = Run(torch, case, slice(c, c + 1), ld).init().step(2)
            assert torch.equal(alone.column_bits(0), full.column_bits(c)), (c, ld)
            assert alone.padding_is_untouched()
    assert wide.padding_is_untouched()


@pytest.mark.parametrize("frozen", [1, 2])
def test_a_stopped_column_is_frozen(case, torch, frozen):
    clean = Run(torch, case, slice(0, QMAX)).init().step(2)
    run = Run(torch, case, slice(0, QMAX)).init().step()
    stopped = (0, 5, 63, 64)
    for c in stopped:
        run.set_status(c, frozen)
    before = [run.column_bits(c).clone() for c in stopped]
    run.step()
    for c, was in zip(stopped, before):
        assert torch.equal(run.column_bits(c), was), c
    assert np.all(run.row("status")[list(stopped)] == frozen) and np.all(run.row("alpha")[list(stopped)] == 0.0)
    for c in (1, 4, 6, 62):   # the running neighbours advance, with the bits of an undisturbed run
        assert run.row("iters")[c] == 2 and torch.equal(run.column_bits(c), clean.column_bits(c))


def test_a_converged_column_stops_on_its_own_and_a_zero_one_at_once(sc, torch):
    case = case_of(sc, torch, ("A", False, 3))
    rhs = case["fd"][:, :4].clone()
    rhs[:, 2] = 0.0
    run = Run(torch, case, slice(0, 4), rhs=rhs).init(tol=0.5)   # (half the norm: a few iterations)
    assert list(run.row("status")) == [0, 0, 1, 0]
    run.step(12)
    iters = run.row("iters")
    assert list(run.row("status")) == [1, 1, 1, 1] and iters[2] == 0 and np.all(iters[[0, 1, 3]] < 12)
    assert np.all(run.row("rho") <= run.row("stop")) and bool((run.X[:, 2] == 0).all())
    after = [run.column_bits(c).clone() for c in range(4)]
    run.step(3)   # further iterations change nothing
    assert all(torch.equal(run.column_bits(c), after[c]) for c in range(4))
    # a column that breaks down: <p, H p> is not positive for a null vector
    null = case["op"].null_space()[:, :1].contiguous()
    bad = Run(torch, case, slice(0, 1), rhs=null).init().step()
    assert bad.row("iters")[0] <= 1 and bool(torch.isfinite(bad.X[:, 0]).all())


@pytest.mark.parametrize("dim", [3, 1])
def test_an_atom_without_pairs_adds_exactly_zero(sc, torch, dim):
    case = case_of(sc, torch, ("n40iso", False, dim))
    assert np.bincount(case["op"].pairs[:, 0], minlength=case["n"])[ISOLATED] == 0
    run = Run(torch, case, slice(0, QMAX), QMAX + 3).init().step()
    rows = slice(dim * ISOLATED, dim * ISOLATED + dim)
    assert bool((run.Q[rows, :QMAX] == 0.0).all())
    assert np.all(np.isfinite(run.row("pq"))) and np.all(np.isfinite(run.row("rho"))) and np.all(run.row("pq") > 0)
    q = run.Q[:, :QMAX].cpu().numpy()
    assert np.all(np.abs(run.row("pq") - (case["f"] * q).sum(axis=0)) <= case["m"] * 2.0 ** -52 * np.abs(case["f"] * q).sum(axis=0))


def test_invalid_arguments_are_refused_before_a_launch(sc, torch):
    from springcraft_amd import _hip

    case = case_of(sc, torch, ("A", False, 3))
    run = Run(torch, case, slice(0, 5), 8)
    op, L, p, bad = run.op, run.L, run.p, _hip.SC_ERR_INVALID_ARG
    size = C.c_size_t()
    assert L.sc_dev_pairs_cg_workspace(0, 5, C.byref(size)) == bad and L.sc_dev_pairs_cg_workspace(120, -1, C.byref(size)) == bad
    assert L.sc_dev_pairs_cg_workspace(120, 5, None) == bad

    def init(n=op.n_atoms, dim=3, x=run.X, r=run.R, pp=run.P, ld=8, q=5, tol=TOL, state=run.state, work=run.work, size=run.bytes):
        return L.sc_dev_pairs_cg_init_f64(op.ctx.handle, n, dim, p(x), p(r), p(pp), ld, q, tol, p(state), p(work), size)

    def step(coord=op._coord, dim=3, pairs=op._pairs, start=op._row_start, x=run.X, r=run.R, pp=run.P, qq=run.Q, ld=8, q=5,
             state=run.state, work=run.work, size=run.bytes, iterations=1):
        return L.sc_dev_pairs_cg_step_f64(op.ctx.handle, p(coord), op.n_atoms, dim, p(pairs), op.n_pairs, p(op._gamma),
                                          p(start), None, p(x), p(r), p(pp), p(qq), ld, q, p(state), p(work), size, iterations)

    assert init(dim=2) == bad and init(n=0) == bad and init(q=-1) == bad and init(ld=4) == bad
    assert init(tol=0.0) == bad and init(tol=float("nan")) == bad
    assert init(x=None) == bad and init(state=None) == bad and init(work=None) == bad and init(size=run.bytes - 8) == bad
    assert init(pp=run.R) == bad and init(x=run.P) == bad
    assert step(dim=2) == bad and step(coord=None) == bad and step(pairs=None) == bad and step(start=None) == bad
    assert step(ld=4) == bad and step(q=-1) == bad and step(iterations=-1) == bad and step(size=run.bytes - 8) == bad
    assert step(qq=None) == bad and step(qq=run.P) == bad and step(x=run.R) == bad and step(state=None) == bad
    torch.cuda.synchronize()
    for t in (run.X, run.P, run.Q, run.state, run.work):
        assert bool((t == SENTINEL).all()), "a refused call wrote"
    assert init(q=0) == _hip.SC_OK and step(q=0) == _hip.SC_OK and init() == _hip.SC_OK and step(iterations=0) == _hip.SC_OK
    torch.cuda.synchronize()
    assert bool((run.Q == SENTINEL).all()) and run.padding_is_untouched()
