"""
The partial spectrum (``subset_by_index``; BASELINE config 5) across batches, clusters and the boundaries of its paths.

After the tridiagonalisation the range solve runs kernels of its own (stein.hip, bt2.hip): k_sturm_range
(multisection on the Sturm count), k_stein (inverse iteration, 4 steps from a hashed start vector, members of a run of
near-equal eigenvalues shifted apart by 10 run eps |T|), CholQR2 (k_chol_inv and two grouped GEMMs, twice) and the
back-transformation of m columns only (k_bt2_wave when ceil(m / 64) batch <= 16, else k_bt2_apply; then
backtransform_batched with ncols = m).  Every member of a batch has its own slice of each of them.

References: LAPACK (numpy / scipy) up to n = 1500, scipy's eigh_tridiagonal for tridiagonal inputs, the closed-form
lattice spectra (tests/util.py) at the orders of config 5.  Gates on every case (none looser than test_eigh_gpu.py's;
tests/util.py:subspace_error states the subspace check):
  - eigenvalues within 1e-11 max|lambda| of the reference (1e-13 for tridiagonal inputs), ascending;
  - largest column residual <= 1e-10 lambda_max, ||V V^T - I||_max <= 1e-10;
  - the subspace: the reference spectrum is split into clusters at gaps of 1e-3 lambda_max; the selected vectors must lie
    in the reference's invariant subspace of the clusters the range touches, to the residual-over-gap bound
    (Davis-Kahan).  When the range holds whole clusters this is ||P - P_ref||_2; when lo / hi cut a cluster it is
    ||(I - P_cluster) v||.
The figures are printed (``pytest -s``).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import (LATTICE_CUTOFF, anm_exact, clustered_spectrum, device_checks, forced_two_stage, gnm_exact,
                        glued_wilkinson, lattice, permute, random_orthogonal, signed_permutation, subspace_error,
                        synthetic_coord, tridiagonal)

pytestmark = pytest.mark.gpu

TOL_W, TOL_W_TRI = 1e-11, 1e-13
TOL_RES, TOL_ORTH = 1e-10, 1e-10


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


def _sym(seed, n, scale=1.0):
    a = np.random.RandomState(seed).randn(n, n)
    return (a + a.T) * scale


_REF = {}


def _reference(a, key=None):
    """LAPACK eigenpairs of `a` (columns), cached by `key`."""
    if key is not None and key in _REF:
        return _REF[key]
    w, v = np.linalg.eigh(a)
    if key is not None:
        _REF[key] = (w, v)
    return w, v


def _gate(label, a, lo, hi, w, v=None, ref=None, tol_w=TOL_W, scale=None):
    """
    All gates on the eigenpairs (w, v) = range [lo, hi] of the symmetric matrix `a` (host, n <= 2000); `ref` = (w_ref,
    v_ref) of LAPACK (computed if None).  Returns the figures.
    """
    w = np.asarray(w)
    w_ref, v_ref = _reference(a) if ref is None else ref
    scale = np.abs(w_ref).max() if scale is None else scale
    m = hi - lo + 1
    assert w.shape == (m,), (label, w.shape)
    out = {"eig": float(np.abs(w - w_ref[lo:hi + 1]).max() / scale)}
    assert out["eig"] <= tol_w, (label, out)
    assert np.all(np.diff(w) >= 0), f"{label}: eigenvalues not ascending"
    if v is not None:
        v = np.asarray(v)
        assert v.shape == (m, len(a)), (label, v.shape)
        r = a @ v.T - v.T * w[None, :]
        out["res"] = float(np.linalg.norm(r, axis=0).max() / scale)
        out["orth"] = float(np.abs(v @ v.T - np.eye(m)).max())
        sub, bound, (a0, b0) = subspace_error(a, w_ref, v_ref, lo, hi, v, np.linalg.norm(r))
        out["sub"], out["sub_bound"] = float(sub), float(bound)
        out["cluster"] = "whole" if (a0, b0) == (lo, hi) else f"cut {a0}..{b0}"
        assert out["res"] <= TOL_RES and out["orth"] <= TOL_ORTH, (label, out)
        assert out["sub"] <= out["sub_bound"], (label, out)
    print(f"{label}: " + ", ".join(f"{k} {x:.1e}" if isinstance(x, float) else f"{k} {x}" for k, x in out.items()))
    return out


# ---- the C ABI entry point: batches ------------------------------------------------------------------------------

class _Solver:
    """sc_dev_eigh_range_f64 on a context of its own, with the tridiagonalisation path forced or automatic."""

    def __init__(self, two_stage):
        import torch

        from springcraft_amd import _hip

        self.torch, self.L = torch, _hip.lib()
        self.ctx = _hip.Context(0)
        self.ctx.set_two_stage(two_stage)

    def close(self):
        self.ctx.close()

    def enqueue(self, mats, lo, hi, vectors=True):
        torch = self.torch
        mats = np.asarray(mats, dtype=np.float64)
        batch, n = mats.shape[0], mats.shape[-1]
        m = hi - lo + 1
        a = torch.from_numpy(mats.copy()).cuda()
        w = torch.full((batch, m), -7.0, dtype=torch.float64, device="cuda")
        v = torch.full((batch, m, n), -7.0, dtype=torch.float64, device="cuda") if vectors else None
        torch.cuda.synchronize()          # (the context has a stream of its own)
        self.ctx.check(self.L.sc_dev_eigh_range_f64(self.ctx.handle, C.c_void_p(a.data_ptr()), n, batch, lo, hi,
                                                    C.c_void_p(w.data_ptr()),
                                                    C.c_void_p(v.data_ptr()) if vectors else None))
        return a, w, v

    def solve(self, mats, lo, hi, vectors=True):
        _, w, v = self.enqueue(mats, lo, hi, vectors)
        self.ctx.synchronize()
        return w.cpu().numpy(), (v.cpu().numpy() if vectors else None)


def _mode_id(mode):
    return {False: "one_stage", True: "two_stage", None: "auto"}[mode]


def _batched_case(mode, n, batch, lo, hi):
    label = f"n={n} batch={batch} [{lo}, {hi}] m={hi - lo + 1} {_mode_id(mode)}"
    mats = np.stack([_sym(1000 * n + b, n) for b in range(batch)])
    solver = _Solver(mode)
    try:
        w, v = solver.solve(mats, lo, hi)
        scale = 0.0
        for b in range(batch):
            ref = _reference(mats[b], (n, b))
            _gate(f"{label} member {b}", mats[b], lo, hi, w[b], v[b], ref)
            scale = max(scale, np.abs(ref[0]).max())
        # each member as the batch-1 solve of the same matrix gives it (the first and the last member)
        for b in sorted({0, batch - 1}):
            w1, _ = solver.solve(mats[b:b + 1], lo, hi)
            assert np.abs(w1[0] - w[b]).max() <= 1e-12 * scale, (label, b)
        # bit for bit on a repeat, and the eigenvalues-only form
        w2, v2 = solver.solve(mats, lo, hi)
        assert np.array_equal(w2, w) and np.array_equal(v2, v), f"{label}: a repeated solve differs"
        w3, _ = solver.solve(mats, lo, hi, vectors=False)
        assert np.abs(w3 - w).max() <= 1e-12 * scale, label
    finally:
        solver.close()


@pytest.mark.parametrize("mode", [False, None], ids=_mode_id)
@pytest.mark.parametrize("n", [300, 513])
@pytest.mark.parametrize("where", ["low", "middle", "high"])
def test_batched_one_stage_orders(mode, n, where):
    """Batch 3 at n = 300 / 513: the one-stage path, forced and by the automatic rule."""
    lo, hi = {"low": (0, 9), "middle": (n // 2 - 20, n // 2 + 17), "high": (n - 64, n - 1)}[where]
    _batched_case(mode, n, 3, lo, hi)


# (batch, m) on both sides of ceil(m / 64) batch = 16 (k_bt2_wave / k_bt2_apply), and 9 matrices for the apply kernel's
# XCD grid (batch >= 8); the automatic rule once per order (two-stage at 1500 x 8 and 512 x 16, one-stage at 1001 x 4)
BATCH_COLS = [(4, 256), (4, 257), (8, 128), (8, 129), (16, 64), (16, 65), (9, 129)]
TWO_STAGE_CASES = [(n, b, m, True) for n in (512, 1001, 1500) for b, m in BATCH_COLS] + [
    (1500, 8, 129, None), (1001, 4, 257, None), (512, 16, 65, None)]


@pytest.mark.parametrize("n,batch,m,mode", TWO_STAGE_CASES,
                         ids=[f"n{n}-b{b}-m{m}-{_mode_id(mode)}" for n, b, m, mode in TWO_STAGE_CASES])
def test_batched_two_stage_column_counts(n, batch, m, mode):
    lo = (n - m) // 3
    _batched_case(mode, n, batch, lo, lo + m - 1)


@pytest.mark.parametrize("two_stage", [False, True])
def test_batched_members_of_very_different_scales(two_stage):
    """Members scaled by 1e-150, 1 and 1e150 in one batch: each is solved to its own scale (unscale_values_batched)."""
    n, lo, hi = 600, 290, 400
    base = [_sym(77 + b, n) for b in range(3)]
    scales = (1e-150, 1.0, 1e150)
    s = _Solver(two_stage)
    try:
        w, v = s.solve(np.stack([a * f for a, f in zip(base, scales)]), lo, hi)
    finally:
        s.close()
    for b, f in enumerate(scales):
        _gate(f"scaled {f:g} {two_stage}", base[b], lo, hi, w[b] / f, v[b])


@pytest.mark.parametrize("two_stage", [False, True])
def test_batched_nan_member(two_stage):
    """A NaN in one member: LinAlgError once at the synchronisation, the other members are what they are alone."""
    n, lo, hi = 520, 0, 70
    mats = np.stack([_sym(31 + b, n) for b in range(4)])
    mats[2, 300, 17] = np.nan
    s = _Solver(two_stage)
    try:
        _, w, v = s.enqueue(mats, lo, hi)
        with pytest.raises(np.linalg.LinAlgError):
            s.ctx.synchronize()
        s.ctx.synchronize()                       # reported once
        w, v = w.cpu().numpy(), v.cpu().numpy()
    finally:
        s.close()
    for b in (0, 1, 3):
        _gate(f"nan batch member {b} {two_stage}", mats[b], lo, hi, w[b], v[b])


# ---- DeviceBatchSolver -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("two_stage", [False, True, None], ids=_mode_id)
def test_device_batch_solver_anm(sc, two_stage):
    """6 structures x 300 atoms, ANM (InvariantForceField 13 A), modes 0..105 with the six rigid-body ones."""
    import torch

    from oracle import enm_oracle as orc
    from springcraft_amd.batch import DeviceBatchSolver

    batch, natoms, lo, hi = 6, 300, 0, 105
    coords = np.stack([synthetic_coord(natoms, 40 + b) for b in range(batch)])
    solver = DeviceBatchSolver(natoms, batch, sc.InvariantForceField(13.0), subset_by_index=(lo, hi))
    solver.ctx.set_two_stage(two_stage)
    solver.solve(torch.from_numpy(coords).cuda())
    w, v = (t.cpu().numpy() for t in solver.finish())
    values_only = DeviceBatchSolver(natoms, batch, sc.InvariantForceField(13.0), want_vectors=False,
                                    subset_by_index=(lo, hi))
    values_only.ctx.set_two_stage(two_stage)
    values_only.solve(torch.from_numpy(coords).cuda())
    w_only = values_only.finish()[0].cpu().numpy()
    assert values_only.v is None
    for b in range(batch):
        h, _ = orc.compute_hessian(coords[b], orc.invariant_ff(13.0))
        ref = _reference(h)
        _gate(f"DeviceBatchSolver ANM {b} {two_stage}", h, lo, hi, w[b], v[b], ref)
        # the 6-dimensional null space on its own: eigenvalues, residual and subspace
        scale = np.abs(ref[0]).max()
        assert np.abs(w[b, :6]).max() <= 1e-11 * scale and w[b, 6] > 1e-6 * scale
        _gate(f"DeviceBatchSolver ANM {b} null space {two_stage}", h, 0, 5, w[b, :6], v[b, :6], ref)
        _gate(f"DeviceBatchSolver ANM {b} values only {two_stage}", h, lo, hi, w_only[b], ref=ref)


def test_device_batch_solver_gnm(sc):
    import torch

    from oracle import enm_oracle as orc
    from springcraft_amd.batch import DeviceBatchSolver

    batch, natoms, lo, hi = 3, 700, 1, 120
    coords = np.stack([synthetic_coord(natoms, 60 + b) for b in range(batch)])
    solver = DeviceBatchSolver(natoms, batch, sc.InvariantForceField(7.0), dim=1, subset_by_index=(lo, hi))
    solver.solve(torch.from_numpy(coords).cuda())
    w, v = (t.cpu().numpy() for t in solver.finish())
    for b in range(batch):
        k, _ = orc.compute_kirchhoff(coords[b], orc.invariant_ff(7.0))
        _gate(f"DeviceBatchSolver GNM {b}", k, lo, hi, w[b], v[b])


# ---- edges of m, one matrix --------------------------------------------------------------------------------------

EDGES = [
    (300, 0, 0), (300, 150, 150), (300, 299, 299),     # lo = hi at both ends and in the middle
    (300, 0, 299),                                      # m = n
    (700, 200, 499),                                    # m = 300: k_chol_inv with more columns than threads
    (1500, 100, 1123), (1500, 100, 1124),               # m = 1024 / 1025: k_bt2_wave / k_bt2_apply
]


@pytest.mark.parametrize("n,lo,hi", EDGES)
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_edges_of_m(two_stage, n, lo, hi):
    a = _sym(5000 + n, n)
    s = _Solver(two_stage)
    try:
        w, v = s.solve(a[None], lo, hi)
    finally:
        s.close()
    _gate(f"n={n} [{lo}, {hi}] m={hi - lo + 1} {two_stage}", a, lo, hi, w[0], v[0], _reference(a, ("edge", n)))


# ---- clusters, one matrix ----------------------------------------------------------------------------------------

W21_BLOCKS = 16                      # n = 336: top clusters of 32 (indices 304..335, 272..303, ...)
W21_RANGES = [(272, 335), (304, 335), (290, 320), (316, 335), (310, 310), (0, 40)]


@pytest.mark.parametrize("glue", [1e-4, 1e-8, 1e-12, 1e-14])
@pytest.mark.parametrize("permuted", [False, True], ids=["tridiagonal", "permuted"])
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_glued_wilkinson(two_stage, permuted, glue):
    """Glued W21^+: clusters of 32 eigenvalues spread by ~glue; ranges that hold whole clusters and that cut them."""
    from scipy.linalg import eigh_tridiagonal

    d, e = glued_wilkinson(W21_BLOCKS, glue)
    n = len(d)
    t = tridiagonal(d, e)
    w_ref, v_ref = _reference(t, ("w21", glue))
    a, ref = t, (w_ref, v_ref)
    if permuted:
        perm, signs = signed_permutation(3, n)
        a = permute(t, perm, signs)
        ref = (w_ref, (v_ref * signs[:, None])[perm])
    s = _Solver(two_stage)
    try:
        for lo, hi in W21_RANGES:
            w, v = s.solve(a[None], lo, hi)
            tri_ref = eigh_tridiagonal(d, e, eigvals_only=True, select="i", select_range=(lo, hi))
            scale = np.abs(w_ref).max()
            assert np.abs(w[0] - tri_ref).max() <= (TOL_W if permuted else TOL_W_TRI) * scale
            _gate(f"W21 glue {glue:g} [{lo}, {hi}] {'permuted' if permuted else 'tridiagonal'} {two_stage}", a, lo,
                  hi, w[0], v[0], ref, tol_w=TOL_W if permuted else TOL_W_TRI)
    finally:
        s.close()


@pytest.mark.parametrize("rel_spacing", [0.0, 1e-13, 1e-10, 1e-7])
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_clusters_of_a_known_spectrum(two_stage, rel_spacing):
    """Q diag(lambda) Q^T with clusters of up to 20 exactly equal or close eigenvalues; lo / hi inside clusters."""
    n = 600
    lam = clustered_spectrum(rel_spacing, seed=2, n=n)
    q = random_orthogonal(8, n)
    a = (q * lam[None, :]) @ q.T
    a = 0.5 * (a + a.T)
    ref = _reference(a)
    scale = np.abs(ref[0]).max()
    assert np.abs(ref[0] - lam).max() <= 1e-12 * scale
    # cluster boundaries of the known spectrum: ranges that start / end inside the 20-, 12- and 8-member clusters
    starts = np.concatenate([[0], np.where(np.diff(lam) > 1e-3 * scale)[0] + 1])
    sizes = np.diff(np.concatenate([starts, [n]]))
    big = [int(s0) for s0, sz in zip(starts, sizes) if sz >= 8]
    assert len(big) >= 3
    ranges = [(big[0], big[0] + 11), (big[0] + 3, big[1] + 4), (big[2] + 1, big[2] + 1), (max(0, big[1] - 5),
              big[1] + int(sizes[list(starts).index(big[1])]) + 4)]
    s = _Solver(two_stage)
    try:
        for lo, hi in ranges:
            w, v = s.solve(a[None], lo, hi)
            _gate(f"clusters spacing {rel_spacing:g} [{lo}, {hi}] {two_stage}", a, lo, hi, w[0], v[0], ref)
    finally:
        s.close()


# ---- lattices at the orders of config 5 ---------------------------------------------------------------------------

def _path_overridden():
    """The path assertions hold for the automatic rules only (tools/test_matrix.sh forces paths through these)."""
    if forced_two_stage() is not None:
        return True
    return any(k.startswith("SPRINGCRAFT_BULGE_") or k.startswith("SPRINGCRAFT_RESIDENT") for k in os.environ)


def _counters(ctx):
    return {k: ctx.counter(k) for k in ("chase_launches", "resident_launches", "chase_timeouts")}


def _check_path(before, after, n):
    if _path_overridden():
        return
    d = {k: after[k] - before[k] for k in after}
    if n <= 7000:
        assert d["resident_launches"] == 1 and d["chase_launches"] == 0, d
    else:
        assert d["chase_launches"] == 1 and d["resident_launches"] == 0, d
    assert d["chase_timeouts"] == 0, d


def _lattice_case(sc, dims, dim, ranges, label):
    import torch

    from springcraft_amd import _hip
    from springcraft_amd.batch import DeviceBatchSolver

    a, b, c = dims
    coord = lattice(a, b, c, sum(dims))
    natoms = len(coord)
    ff = sc.InvariantForceField(LATTICE_CUTOFF)
    exact = np.sort(anm_exact(a, b, c) if dim == 3 else gnm_exact(a, b, c)).astype(np.float64)
    scale = float(np.abs(exact).max())
    assembler = DeviceBatchSolver(natoms, 1, ff, dim=dim, want_vectors=False)
    h = assembler.assemble(torch.from_numpy(coord[None]).cuda())[0]
    torch.cuda.synchronize()
    ctx = _hip.context()
    model = sc.ANM(coord, ff) if dim == 3 else sc.GNM(coord, ff)
    for lo, hi in ranges:
        before = _counters(ctx)
        w, v = model.eigen(subset_by_index=(lo, hi))
        _check_path(before, _counters(ctx), natoms * dim)
        w = np.asarray(w)
        eig = float(np.abs(w - exact[lo:hi + 1]).max() / scale)
        assert np.all(np.diff(w) >= 0), (label, lo, hi)
        res, orth = device_checks(torch, h, torch.from_numpy(w).cuda(), torch.from_numpy(np.asarray(v)).cuda(),
                                  scale=scale)
        print(f"{label} [{lo}, {hi}] m={hi - lo + 1}: eig {eig:.1e}, res {res:.1e}, orth {orth:.1e}")
        assert eig <= TOL_W and res <= TOL_RES and orth <= TOL_ORTH, (label, lo, hi, eig, res, orth)
        del v


def test_anm_lattice_c5_order(sc):
    """20 x 20 x 20 ANM lattice (n = 24000): 1200 exact zeros, then 1200-fold clusters.  (0, 105) is config 5's call,
    (1150, 1255) straddles the zeros and the first cluster, (1190, 2410) takes the apply path and a large CholQR."""
    _lattice_case(sc, (20, 20, 20), 3, [(0, 105), (1150, 1255), (1190, 2410)], "ANM lattice n=24000")


def test_gnm_lattice_n8000(sc):
    """20 x 20 x 20 GNM lattice: sums of three path spectra, many exact and near-exact ties."""
    _lattice_case(sc, (20, 20, 20), 1, [(0, 299)], "GNM lattice n=8000")


def test_anm_lattice_one_stage(sc):
    """12 x 12 x 12 ANM lattice (n = 5184): one-stage, the trailing matrix in one resident launch; 432 exact zeros."""
    _lattice_case(sc, (12, 12, 12), 3, [(0, 105), (400, 700)], "ANM lattice n=5184")
