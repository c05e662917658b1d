"""
Full-spectrum solves above the divide & conquer's LDS limits (orders 7000 .. 9900).

Below n = 7000 every merge of the D&C keeps its sorted copies (k_dc_setup, 22 B per element) and its poles
(k_dc_secular, 16 B per pole) in LDS; from 7001 / 9801 on the top merge works from global scratch (stedc.hip,
kLdsCapSetup / kLdsCapSecular), and one matrix goes two-stage from 7001 on (eigh_policy.h, two_stage_for) -- the path
``ANM(coord, ff).eigen()`` takes for a structure of more than 2333 residues.  The references are exact in closed form
wherever possible: elastic networks on a cubic lattice (spacing 3.8 A, cutoff 4.5 A: only axis neighbours are in
contact) have the spectra of sums of path graphs,
  - GNM Kirchhoff = Laplacian of the a x b x c grid graph: {p_a(i) + p_b(j) + p_c(k)},
  - ANM Hessian (gamma = 1): p_a with multiplicity b c, p_b with a c, p_c with a b (a bond along axis d only couples
    displacements along d; the rotation of the lattice is a similarity), ab + bc + ca exact zeros,
with p_m(k) = 4 sin^2(pi k / 2m).  The random and Hinsen cases compare with host LAPACK (tests/golden/generated/
large_order_eigvalsh.npz, oracle/make_large_order_golden.py) or, at n = 9801, with the eigenvalues-only path.
Gates: the suite's tight ones (1e-11), for all n eigenpairs, computed on the device.
"""
import math
import os

import numpy as np
import pytest

from tests.util import LATTICE_CUTOFF as CUTOFF
from tests.util import LATTICE_SPACING as SPACING
from tests.util import anm_exact as _anm_exact
from tests.util import device_checks, forced_two_stage, generated, synthetic_coord
from tests.util import gnm_exact as _gnm_exact
from tests.util import lattice as _lattice
from tests.util import path_eigs as _path_eigs

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


def _path_overridden():
    """The path assertions hold for the automatic rules only (tools/test_matrix.sh forces paths through these)."""
    if forced_two_stage() is not None:
        return True
    return any(k.startswith("SPRINGCRAFT_BULGE_") or k.startswith("SPRINGCRAFT_RESIDENT") for k in os.environ)


def _chain(m, offset):
    """m points on a straight line (spacing 3.8 A), far from everything else."""
    return np.arange(m)[:, None] * np.array([SPACING, 0.0, 0.0]) + np.asarray(offset, dtype=np.float64)


def _grid_laplacian(a, b, c):
    """Laplacian of the a x b x c grid graph (vertex order of _lattice), from the indices alone."""
    n = a * b * c
    idx = np.arange(n).reshape(a, b, c)
    lap = np.zeros((n, n))
    for lo, hi in ((idx[:-1], idx[1:]), (idx[:, :-1], idx[:, 1:]), (idx[:, :, :-1], idx[:, :, 1:])):
        lap[lo.ravel(), hi.ravel()] = -1.0
        lap[hi.ravel(), lo.ravel()] = -1.0
    lap[np.arange(n), np.arange(n)] = -lap.sum(axis=1)
    return lap


def _counters(ctx):
    names = ("chase_launches", "stepwise_chases", "chase_sweeps", "resident_launches", "chase_timeouts",
             "chase_resumed", "chase_incomplete")
    return {k: ctx.counter(k) for k in names}


def _check_path(before, after, n):
    if _path_overridden():
        return
    d = {k: after[k] - before[k] for k in after}
    if n <= 7000:
        assert d["resident_launches"] == 1 and d["chase_launches"] == 0, d
    else:
        assert d["chase_launches"] == 1 and d["stepwise_chases"] == 0 and d["chase_sweeps"] == n - 2, d
    assert d["chase_timeouts"] == 0 and d["chase_resumed"] == 0 and d["chase_incomplete"] == 0, d


def _certify(torch, label, a, w, v, ref=None, zeros=None):
    """
    a: (n, n) float64 CUDA tensor, w: (n,) host eigenvalues, v: (n, n) CUDA tensor (rows = modes).  Gates: eigenvalues
    against `ref` (closed form or LAPACK) to 1e-11 lambda_max, the count of |w| <= 1e-11 lambda_max equals `zeros`,
    residual of every pair <= 1e-11 ||A||_2, ||V V^T - I||_max <= 1e-11, sum w = tr A and sum w^2 = ||A||_F^2 to 1e-12.
    """
    w = np.asarray(w, dtype=np.float64)
    lam_max = float(np.abs(w).max())
    assert np.all(np.diff(w) >= 0), f"{label}: eigenvalues not ascending"
    out = {}
    if ref is not None:
        ref = np.sort(np.asarray(ref, dtype=np.longdouble)).astype(np.float64)
        out["eig_err"] = float(np.abs(w - ref).max() / np.abs(ref).max())
        assert out["eig_err"] <= TOL, (label, out)
    if zeros is not None:
        out["zeros"] = int(np.sum(np.abs(w) <= TOL * lam_max))
        assert out["zeros"] == zeros, (label, out, zeros)
    tr = float(torch.trace(a))
    fro2 = float((a * a).sum())
    out["trace_err"] = abs(math.fsum(w) - tr) / math.fsum(np.abs(w))
    out["fro_err"] = abs(math.fsum(w * w) - fro2) / fro2
    assert out["trace_err"] <= 1e-12 and out["fro_err"] <= 1e-12, (label, out)
    out["res"], out["orth"] = device_checks(torch, a, torch.from_numpy(w).to(a.device), v)
    assert out["res"] <= TOL and out["orth"] <= TOL, (label, out)
    print(f"{label}: " + ", ".join(f"{k} {x:.2e}" if isinstance(x, float) else f"{k} {x}" for k, x in out.items()))
    return out


def _values_only(sc, matrix, ref, label):
    w = sc.nma.eigh(matrix, eigenvectors=False)
    err = float(np.abs(w - ref).max() / np.abs(ref).max())
    print(f"{label} (eigenvalues only): eig_err {err:.2e}")
    assert err <= TOL, (label, err)


GNM_CASES = {
    # order: (lattice dims, atoms of the far straight chain)
    7000: ((14, 20, 25), 0),     # one-stage + resident trailing launch; k_dc_setup at its largest LDS request
    7001: ((20, 20, 17), 201),   # two-stage, spread chase; setup from global scratch; block-diagonal input
    9800: ((14, 25, 28), 0),     # setup global, k_dc_secular at its largest LDS request
    9801: ((9, 11, 99), 0),      # setup and secular both global
}


@pytest.mark.parametrize("n", sorted(GNM_CASES))
def test_gnm_lattice(sc, n):
    """GNM Kirchhoff of a rotated grid (plus a far chain at 7001): exact Laplacian, exact spectrum, all eigenpairs."""
    import torch

    from springcraft_amd import _hip

    (a, b, c), m = GNM_CASES[n]
    coord = _lattice(a, b, c, n)
    lap = _grid_laplacian(a, b, c)
    exact = _gnm_exact(a, b, c)
    zeros = 1
    if m:
        coord = np.concatenate([coord, _chain(m, (-2000.0, 500.0, 100.0))])
        pl = _grid_laplacian(m, 1, 1)
        lap = np.block([[lap, np.zeros((len(lap), m))], [np.zeros((m, len(lap))), pl]])
        exact = np.concatenate([exact, _path_eigs(m).astype(np.longdouble)])
        zeros = 2
    assert len(coord) == n
    kirchhoff = sc.GNM(coord, sc.InvariantForceField(CUTOFF)).kirchhoff
    assert np.array_equal(kirchhoff, lap)   # the large-N contact scan finds exactly the axis neighbours
    ctx = _hip.context()
    before = _counters(ctx)
    w, v = sc.nma.eigh(kirchhoff)
    _check_path(before, _counters(ctx), n)
    ad = torch.from_numpy(lap).cuda()
    _certify(torch, f"GNM n={n}", ad, w, torch.from_numpy(np.asarray(v)).cuda(), ref=exact, zeros=zeros)
    _values_only(sc, kirchhoff, np.sort(exact).astype(np.float64), f"GNM n={n}")


ANM_CASES = {7200: (12, 10, 20), 9900: (10, 15, 22)}


@pytest.mark.parametrize("n", sorted(ANM_CASES))
def test_anm_lattice(sc, n):
    """ANM (gamma = 1) of a rotated grid through ``ANM(coord, ff).eigen()``: ab + bc + ca exact zero modes."""
    import torch

    from springcraft_amd import _hip

    a, b, c = ANM_CASES[n]
    coord = _lattice(a, b, c, n)
    ff = sc.InvariantForceField(CUTOFF)
    exact = _anm_exact(a, b, c)
    ctx = _hip.context()
    before = _counters(ctx)
    w, v = sc.ANM(coord, ff).eigen()
    _check_path(before, _counters(ctx), n)
    hessian = sc.ANM(coord, ff).hessian
    _certify(torch, f"ANM lattice n={n}", torch.from_numpy(hessian).cuda(), w, torch.from_numpy(np.asarray(v)).cuda(),
             ref=exact, zeros=a * b + b * c + c * a)
    _values_only(sc, hessian, np.sort(exact), f"ANM lattice n={n}")


@pytest.mark.parametrize("n", [7001, 9801])
def test_random_symmetric_above_lds_limits(sc, n):
    """
    a + a^T: almost no deflation, the secular solver over ~n poles.  7001: against host LAPACK; 9801: the D&C's
    eigenvalues against the eigenvalues-only path (Sturm bisection, no D&C), with residual / orthogonality / trace /
    Frobenius as the certificates.
    """
    import torch

    from springcraft_amd import _hip

    rs = np.random.RandomState(n)
    m = rs.randn(n, n)
    m = m + m.T
    ctx = _hip.context()
    before = _counters(ctx)
    w, v = sc.nma.eigh(m)
    _check_path(before, _counters(ctx), n)
    ref = generated("large_order_eigvalsh.npz")["random_7001"] if n == 7001 else None
    _certify(torch, f"random n={n}", torch.from_numpy(m).cuda(), w, torch.from_numpy(np.asarray(v)).cuda(), ref=ref)
    _values_only(sc, m, ref if ref is not None else w, f"random n={n}")


def test_anm_hinsen_n7200(sc):
    """The user's call on an ordinary large structure: ``ANM(coord, HinsenForceField()).eigen()`` for 2400 atoms."""
    import torch

    from springcraft_amd import _hip

    n = 7200
    coord = synthetic_coord(2400, 24)
    ff = sc.HinsenForceField()
    ref = generated("large_order_eigvalsh.npz")["hinsen_7200"]
    ctx = _hip.context()
    before = _counters(ctx)
    w, v = sc.ANM(coord, ff).eigen()
    _check_path(before, _counters(ctx), n)
    hessian = sc.ANM(coord, ff).hessian
    _certify(torch, "ANM Hinsen n=7200", torch.from_numpy(hessian).cuda(), w, torch.from_numpy(np.asarray(v)).cuda(),
             ref=ref, zeros=6)
    _values_only(sc, hessian, ref, "ANM Hinsen n=7200")


# members (lattice dims, rotation seed): every batch has the first lattice again at position 3 (bit-identical
# eigenvalues); ten members put two DIFFERENT matrices on one XCD (workgroup b of a launch runs on XCD b mod 8), where
# they share an L2 -- on different XCDs a shared scratch can go unnoticed, each XCD's L2 keeping its own copy
BATCHES = {
    4: [(12, 10, 20, 7200), (8, 15, 20, 7200), (6, 20, 20, 7200), (12, 10, 20, 7200)],
    10: [(12, 10, 20, 7200), (8, 15, 20, 7200), (6, 20, 20, 7200), (12, 10, 20, 7200), (10, 12, 20, 1), (8, 10, 30, 2),
         (5, 20, 24, 3), (6, 16, 25, 4), (12, 10, 20, 5), (10, 15, 16, 6)],
}


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_batched_anm_lattices_n7200(sc, batch):
    """
    2400-atom lattices in ONE batched device solve (sc_dev_hessian_f64 + sc_dev_eigh_f64), n = 7200: the D&C's global
    scratch is per matrix (b * 3n).  4 members: the spread chase; 10: one chase form with matrices bound to XCDs.
    Every member meets the gates; members 0 and 3 have bit-identical eigenvalues.
    """
    import torch

    from springcraft_amd.batch import DeviceBatchSolver

    members = BATCHES[batch]
    n_atoms, n = 2400, 7200
    coord = torch.from_numpy(np.stack([_lattice(a, b, c, seed) for a, b, c, seed in members])).cuda()
    ff = sc.InvariantForceField(CUTOFF)
    solver = DeviceBatchSolver(n_atoms, batch, ff)
    hessians = solver.assemble(coord).clone()
    w, v = solver.eigh()
    solver.finish()
    if not _path_overridden():
        cnt = _counters(solver.ctx)
        assert cnt["chase_launches"] == 1 and cnt["stepwise_chases"] == 0, cnt
        assert cnt["chase_sweeps"] == batch * (n - 2) and cnt["chase_resumed"] == 0, cnt
    w_h = w.cpu().numpy()
    assert np.array_equal(w_h[0], w_h[3])
    values_only = DeviceBatchSolver(n_atoms, batch, ff, want_vectors=False)
    w_only, _ = values_only.solve(coord)
    values_only.finish()
    w_only = w_only.cpu().numpy()
    for bi, (a, b, c, _) in enumerate(members):
        exact = _anm_exact(a, b, c)
        _certify(torch, f"batch {batch} member {bi} ({a}x{b}x{c})", hessians[bi], w_h[bi], v[bi], ref=exact,
                 zeros=a * b + b * c + c * a)
        err = float(np.abs(w_only[bi] - np.sort(exact)).max() / exact.max())
        assert err <= TOL, (bi, err)


def test_chase_counters_survive_the_d_and_c_above_7000():
    """
    The persistent chase's control block (tickets per XCD, where a wait timed out) is read at the next synchronising
    call, after the D&C of the same solve -- whose global scratch, for n > 7000, used to share the workspace the block
    sat in.  One full-spectrum solve at n = 7001 on a fresh context: no time-out, no take-over, the wait triple -1, and
    the ticket counts of a one-matrix chase: all workgroups on one ticket slot (the spread form counts as one XCD; so does
    a device with one), 1 <= min <= max = total <= max(8, ceil((n - 1) / 64) / 2 + 1), the workgroups one matrix's chase
    can use (twostage_policy.h, `useful`).  The same order without eigenvectors (no D&C) is the control: same grid.
    """
    import ctypes as C

    import torch

    from springcraft_amd import _hip

    n = 7001
    rs = np.random.RandomState(17)
    m = rs.randn(n, n)
    m = m + m.T
    L = _hip.lib()
    names = ("chase_launches", "chase_timeouts", "chase_incomplete", "chase_resumed", "chase_wait_matrix",
             "chase_wait_sweep", "chase_wait_task", "chase_xcd_min", "chase_xcd_max", "chase_xcd_total")
    runs = {}
    for vectors in (True, False):
        ctx = _hip.Context(0)
        try:
            a = torch.from_numpy(m.copy()).cuda()
            w = torch.empty((1, n), dtype=torch.float64, device="cuda")
            v = torch.empty((1, n, n), dtype=torch.float64, device="cuda") if vectors else None
            torch.cuda.synchronize()
            ctx.check(L.sc_dev_eigh_f64(ctx.handle, C.c_void_p(a.data_ptr()), n, 1, C.c_void_p(w.data_ptr()),
                                        C.c_void_p(v.data_ptr()) if vectors else None))
            ctx.synchronize()
            runs[vectors] = {k: ctx.counter(k) for k in names}
        finally:
            ctx.close()
    print(f"chase counters, n = {n}: with vectors {runs[True]}, eigenvalues only {runs[False]}")
    if _path_overridden():
        return
    bound = max(8, -(-(n - 1) // 64) // 2 + 1)
    for vectors, c in runs.items():
        assert c["chase_launches"] == 1, (vectors, runs)
        assert c["chase_timeouts"] == 0 and c["chase_incomplete"] == 0 and c["chase_resumed"] == 0, (vectors, runs)
        assert (c["chase_wait_matrix"], c["chase_wait_sweep"], c["chase_wait_task"]) == (-1, -1, -1), (vectors, runs)
        assert 1 <= c["chase_xcd_min"] <= c["chase_xcd_max"] <= bound, (vectors, bound, runs)
        assert c["chase_xcd_min"] == c["chase_xcd_max"] == c["chase_xcd_total"], (vectors, runs)
    assert runs[True]["chase_xcd_total"] == runs[False]["chase_xcd_total"], runs
