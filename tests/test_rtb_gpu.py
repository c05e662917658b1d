"""
GPU tests of the rotation-translation-block modes: the projection ``k_rtb_blocks`` and the expansion ``k_rtb_expand`` of
csrc/rtb.hip through ``sc_dev_rtb_hessian_f64`` / ``sc_dev_rtb_expand_f64`` and the public :class:`springcraft_amd.RTB`.

Networks: ``np.random.seed(s); rand(N, 3) * 5 * N**(1/3)`` under ``InvariantForceField(13.0)``, as in
tests/test_mode_response_gpu.py.  Standard blocking: runs of 1, 2, 3, 4, 5, 7 atoms repeating, atoms 3, 4, 5 collinear
(tests/test_rtb_host.py).  For N in {21, 64, 131, 200}, with and without masses ``RandomState(5).uniform(50, 200, N)``,
NumPy gives nr = 31 / 95 / 191 / 293, six trivial |lambda| <= 2.1e-15 lambda_max, lambda_6 / lambda_max >= 0.029 and
lambda_k(H_b) - lambda_k(H) >= -1.8e-15 lambda_max.  Every numeric test asserts on its NumPy spectrum that the trivial
|lambda| <= 1e-13 lambda_max and lambda_6 >= 0.02 lambda_max before it compares anything (``block_spectrum``).

The reference throughout is NumPy on the package's own ``ANM(...).hessian`` and the dense projector assembled from the
solver's ``projector`` / ``offset``.

Tolerances.  Projection: ``atol = 1e-12 max|ref|, rtol = 0``; an entry sums at most about 7 atoms x 200 contacts terms of
size <= max gamma, about 1400 eps = 3e-13 -- the project's Hessian gate, three times that bound.  Expansion: 1e-14
max|ref| (six terms).  Modes: eigenvalues and residuals to 1e-10 lambda_max (the gate of the mode-response tests),
orthonormality and membership of the block space to 1e-12, Rayleigh-Ritz ``w[k] >= lambda_k(H) - 1e-12 lambda_max``.
Consumers are compared with NumPy on the solver's own ``w`` / ``v`` rows with the tolerances of the consumers' own tests:
what is under test there is which rows they take.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_rtb_host import dense_projector, masses_of, network, standard_case
from tests.util import structures

pytestmark = pytest.mark.gpu

CUTOFF = 13.0


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def block_spectrum(ref, random_network=True):
    """
    Ascending eigenvalues of the reference block matrix, with the module docstring's preconditions asserted.  The bound on
    lambda_6 belongs to the random networks; the 1l2y chain under Hinsen's or the eANM constants has lambda_6 / lambda_max
    = 1.2e-3 / 9.9e-3 in NumPy (stiff bonded springs), and there only a projection is compared, which does not depend on it.
    """
    lam = np.linalg.eigvalsh(ref)
    top = np.abs(lam).max()
    assert np.abs(lam[:6]).max() <= 1e-13 * top, "trivial eigenvalues are not at rounding level"
    if random_network:
        assert lam[6] >= 0.02 * top, f"lambda_6 / lambda_max = {lam[6] / top:.3e}: the block network is nearly disconnected"
    else:
        assert lam[6] >= 1e-4 * top, f"lambda_6 / lambda_max = {lam[6] / top:.3e}: more than six trivial modes"
    return lam


def reference(sc, rtb, coord, ff, masses=None):
    """(Pf (3N, nr), H of the package's ANM, Pf^T H Pf)."""
    Pf = dense_projector(rtb.projector, rtb.block_of_atom, rtb.offset)
    h = np.array(sc.ANM(coord, ff, masses=masses).hessian)
    return Pf, h, Pf.T @ h @ Pf


def check_projection(got, ref):
    print(f"max |H_b - ref| / max|ref| = {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    assert got.shape == ref.shape
    assert np.allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


class _Atoms:
    """An atom container around coordinates: ``ANM`` wants one for a mass array."""

    def __init__(self, coord):
        self.coord = coord

    def array_length(self):
        return len(self.coord)


_CACHE = {}


def solved_case(sc, n_atoms):
    """(coord, RTB, Pf, H, reference H_b, its spectrum, the full spectrum): built once per size, read-only."""
    if n_atoms not in _CACHE:
        coord, labels = standard_case(n_atoms)
        ff = sc.InvariantForceField(CUTOFF)
        rtb = sc.RTB(coord, ff, labels)
        Pf, h, ref = reference(sc, rtb, coord, ff)
        lam_b, lam = block_spectrum(ref), np.linalg.eigvalsh(h)
        for a in (coord, Pf, h, ref, lam_b, lam):
            a.setflags(write=False)
        _CACHE[n_atoms] = (coord, rtb, Pf, h, ref, lam_b, lam)
    return _CACHE[n_atoms]


# ---- 1. projection -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [21, 131, 200])
@pytest.mark.parametrize("with_masses", [False, True])
def test_projection_standard_blocking(sc, n_atoms, with_masses):
    coord, labels = standard_case(n_atoms)
    m = masses_of(n_atoms) if with_masses else None
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(_Atoms(coord) if with_masses else coord, ff, labels, masses=m)
    assert rtb.nr == {21: 31, 131: 191, 200: 293}[n_atoms] and list(rtb.dof[:4]) == [3, 5, 5, 6]
    _, _, ref = reference(sc, rtb, _Atoms(coord) if with_masses else coord, ff, m)
    block_spectrum(ref)
    got = rtb.projected_hessian()
    assert got.is_cuda and tuple(got.shape) == (rtb.nr, rtb.nr)
    check_projection(got.cpu().numpy(), ref)


def test_projection_interleaved_labels(sc):
    coord, _ = standard_case(200)
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(coord, ff, np.arange(200) % 40)
    _, _, ref = reference(sc, rtb, coord, ff)
    block_spectrum(ref)
    check_projection(rtb.projected_hessian().cpu().numpy(), ref)


def test_projection_block_larger_than_a_workgroup(sc):
    coord = network(300, 0)
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(coord, ff, np.repeat([0, 1], [270, 30]))
    assert rtb.nr == 12
    _, _, ref = reference(sc, rtb, coord, ff)
    block_spectrum(ref)
    check_projection(rtb.projected_hessian().cpu().numpy(), ref)


def test_projection_one_atom_per_block_is_the_hessian(sc):
    coord = network(64, 0)
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(coord, ff, np.arange(64))
    assert rtb.nr == 192 and np.all(rtb.dof == 3)
    h, _ = sc.compute_hessian(coord, ff)
    block_spectrum(h)
    check_projection(rtb.projected_hessian().cpu().numpy(), h)


def test_projection_one_block_is_zero(sc):
    coord = network(64, 0)
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(coord, ff, np.zeros(64, dtype=int))
    assert rtb.nr == 6
    h, _ = sc.compute_hessian(coord, ff)
    got = rtb.projected_hessian().cpu().numpy()
    print(f"max |H_b| / max|H| = {np.abs(got).max() / np.abs(h).max():.3e}")
    assert got.shape == (6, 6) and np.abs(got).max() <= 1e-13 * np.abs(h).max()


def test_projection_atom_without_contacts(sc):
    coord, labels = standard_case(21)
    coord[20] = coord[:20].mean(axis=0) + 100.0
    labels[20] = labels.max() + 1
    ff = sc.InvariantForceField(CUTOFF)
    rtb = sc.RTB(coord, ff, labels)
    _, _, ref = reference(sc, rtb, coord, ff)
    got = rtb.projected_hessian().cpu().numpy()
    o = int(rtb.offset[rtb.block_of_atom[20]])
    assert rtb.dof[rtb.block_of_atom[20]] == 3 and o == rtb.nr - 3
    assert np.all(got[o:, :] == 0.0) and np.all(got[:, o:] == 0.0)
    check_projection(got, ref)


@pytest.mark.parametrize("ff_name", ["hinsen", "e_anm"])
def test_projection_other_force_fields(sc, ff_name):
    s = structures()
    n = len(s["1l2y_coord"])
    ca = sc.AtomArray(n)
    ca.coord, ca.res_name = s["1l2y_coord"], s["1l2y_res_name"]
    ca.chain_id, ca.res_id = s["1l2y_chain_id"], s["1l2y_res_id"]
    ff = sc.HinsenForceField() if ff_name == "hinsen" else sc.TabulatedForceField.e_anm(ca)
    rtb = sc.RTB(ca, ff, sc.blocks_of_consecutive(n, 4))
    _, _, ref = reference(sc, rtb, ca, ff)
    block_spectrum(ref, random_network=False)
    check_projection(rtb.projected_hessian().cpu().numpy(), ref)


def test_projection_asymmetric_constants(sc):
    """Off-diagonal from gamma(i, j), diagonal summed over the first index: the convention of sc_hessian_from_pairs_f64."""
    from springcraft_amd.forcefield import ForceField

    class Lopsided(ForceField):
        cutoff_distance = CUTOFF

        def force_constant(self, atom_i, atom_j, sq_distance):
            return 1.0 + 0.25 * (atom_i > atom_j) + 0.01 * (atom_i % 7)

    coord, labels = standard_case(64)
    ff = Lopsided()
    rtb = sc.RTB(coord, ff, labels)
    h, _ = sc.compute_hessian(coord, ff)
    assert np.abs(h - h.T).max() > 1e-3
    Pf = dense_projector(rtb.projector, rtb.block_of_atom, rtb.offset)
    check_projection(rtb.projected_hessian().cpu().numpy(), Pf.T @ h @ Pf)


# ---- 2. determinism ------------------------------------------------------------------------------------------------------
def test_bit_identical_from_call_to_call(sc, torch):
    coord, labels = standard_case(131)
    rtb = sc.RTB(coord, sc.InvariantForceField(CUTOFF), labels)
    assert torch.equal(rtb.projected_hessian(), rtb.projected_hessian())
    rtb.solve()
    w1, v1 = (t.clone() for t in rtb.finish())
    rtb.solve()
    w2, v2 = rtb.finish()
    assert torch.equal(w1, w2) and torch.equal(v1, v2)


# ---- 3. expansion alone --------------------------------------------------------------------------------------------------
def test_expansion(sc, torch):
    _, rtb, Pf, *_ = solved_case(sc, 131)
    u = np.random.RandomState(3).standard_normal((7, rtb.nr))
    ref = u @ Pf.T
    d_u = torch.from_numpy(u).to(rtb.device)
    d_v = torch.full((7, 3 * 131), float("nan"), dtype=torch.float64, device=rtb.device)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rtb.ctx.check(rtb._L.sc_dev_rtb_expand_f64(rtb.ctx.handle, p(d_u), 7, rtb.nr, p(rtb._P), p(rtb._boa), p(rtb._offset),
                                               131, p(d_v)))
    rtb.ctx.synchronize()
    got = d_v.cpu().numpy()
    print(f"max |V - ref| / max|ref| = {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    assert np.allclose(got, ref, rtol=0, atol=1e-14 * np.abs(ref).max())


# ---- 4. modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [64, 131, 200])
@pytest.mark.parametrize("subset", [None, (0, 25), (6, 40)])
def test_modes(sc, n_atoms, subset):
    _, rtb, Pf, _, ref, lam_b, lam = solved_case(sc, n_atoms)
    top = lam_b.max()
    w, v = rtb.eigen(subset_by_index=subset)
    lo, hi = (0, rtb.nr - 1) if subset is None else subset
    nvec = hi - lo + 1
    assert w.shape == (nvec,) and v.shape == (nvec, 3 * n_atoms)
    assert tuple(rtb.w.shape) == (1, nvec) and tuple(rtb.v.shape) == (1, nvec, 3 * n_atoms) and rtb._first_row == lo
    u = v @ Pf
    res = np.abs(u @ ref - w[:, None] * u).max()
    print(f"|w - ref| {np.abs(w - lam_b[lo: hi + 1]).max() / top:.2e}  |V V^T - I| {np.abs(v @ v.T - np.eye(nvec)).max():.2e}  "
          f"outside the block space {np.abs(v - u @ Pf.T).max():.2e}  residual {res / top:.2e}")
    assert np.allclose(w, lam_b[lo: hi + 1], rtol=0, atol=1e-10 * top)
    assert np.abs(v @ v.T - np.eye(nvec)).max() <= 1e-12
    assert np.linalg.norm(v - u @ Pf.T, axis=1).max() <= 1e-12
    assert np.linalg.norm(u @ ref - w[:, None] * u, axis=1).max() <= 1e-10 * top
    assert np.all(w >= lam[lo: hi + 1] - 1e-12 * lam.max())


def test_one_atom_per_block_gives_the_anm_spectrum(sc):
    coord = network(64, 0)
    ff = sc.InvariantForceField(CUTOFF)
    w_ref, _ = sc.ANM(coord, ff).eigen()
    block_spectrum(np.diag(w_ref))
    w, v = sc.RTB(coord, ff, np.arange(64)).eigen()
    assert v.shape == (192, 192)
    assert np.allclose(w, w_ref, rtol=0, atol=1e-10 * w_ref.max())


# ---- 5. consumers on the RTB modes ---------------------------------------------------------------------------------------
def test_consumers(sc, torch):
    n = 131
    _, rtb, *_ = solved_case(sc, n)
    rtb.solve()
    w, v = (t[0].cpu().numpy() for t in rtb.finish())
    nr = rtb.nr
    vv = v.reshape(nr, n, 3)
    msf = rtb.mean_square_fluctuation()
    assert tuple(msf.shape) == (1, n)
    assert np.allclose(msf[0].cpu().numpy(), ((vv[6:] ** 2).sum(-1) / w[6:, None]).sum(0))
    sub = np.arange(8, 30)
    assert np.allclose(rtb.mean_square_fluctuation(mode_subset=sub)[0].cpu().numpy(),
                       ((vv[sub] ** 2).sum(-1) / w[sub, None]).sum(0))
    with pytest.raises(ValueError):
        rtb.mean_square_fluctuation(mode_subset=[5, 7])        # a trivial mode
    with pytest.raises(ValueError):
        rtb.mean_square_fluctuation(mode_subset=[nr])          # beyond the block spectrum

    d = np.random.RandomState(11).standard_normal((1, 2, n, 3))
    ov = rtb.overlap(torch.from_numpy(d).to(rtb.device))
    assert tuple(ov.shape) == (1, 2, nr)
    dd = d.reshape(2, -1)
    ref = (dd @ v.T) / (np.linalg.norm(dd, axis=1)[:, None] * np.linalg.norm(v, axis=1)[None, :])
    assert np.allclose(ov[0].cpu().numpy(), ref)

    f = np.random.RandomState(12).standard_normal((1, n, 3))
    x = rtb.linear_response(torch.from_numpy(f).to(rtb.device))
    assert tuple(x.shape) == (1, n, 3)
    keep = np.abs(w) > 1e-6 * np.abs(w).max()
    assert keep.sum() == nr - 6 and not keep[:6].any()
    ref = ((v[keep] @ f.reshape(-1)) / w[keep]) @ v[keep]
    assert np.allclose(x[0].cpu().numpy().reshape(-1), ref, rtol=0, atol=1e-10 * np.abs(ref).max())

    fr = rtb.frequencies()[0].cpu().numpy()
    assert fr.shape == (nr,) and np.all(np.isfinite(fr))
    assert np.allclose(fr[6:], np.sqrt(w[6:]) / (2 * np.pi)) and np.allclose(fr[:6], np.sqrt(np.abs(w[:6])) / (2 * np.pi))


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_errors(sc, torch):
    coord, labels = standard_case(21)
    ff = sc.InvariantForceField(CUTOFF)
    with pytest.raises(IndexError):
        sc.RTB(coord, ff, labels[:-1])
    with pytest.raises(ValueError):
        sc.RTB(coord[:, :2], ff, labels)
    far = coord.copy()
    far[20] += 1000.0
    lonely = sc.RTB(far, ff, labels)
    with pytest.raises(ValueError, match="20"):
        lonely.solve()
    assert lonely.w is None and lonely.v is None            # raised before anything was solved
    rtb = sc.RTB(coord, ff, labels)
    with pytest.raises(ValueError):
        rtb.mean_square_fluctuation()                        # no solve yet
    with pytest.raises(ValueError):
        rtb.solve(subset_by_index=(0, rtb.nr))
    rtb.solve()
    rtb.finish()
    with pytest.raises(ValueError):
        rtb.overlap(torch.zeros((1, 20, 3), dtype=torch.float64, device=rtb.device))
    with pytest.raises(ValueError):
        rtb.linear_response(torch.zeros((21, 3), dtype=torch.float64, device=rtb.device))
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    L, h = rtb._L, rtb.ctx.handle
    out = torch.zeros((rtb.nr, 63), dtype=torch.float64, device=rtb.device)
    for nvec, nr, n_atoms, d_u in [(0, rtb.nr, 21, p(rtb._u)), (rtb.nr, 0, 21, p(rtb._u)), (rtb.nr, rtb.nr, 0, p(rtb._u)),
                                   (rtb.nr, rtb.nr, 21, None)]:
        assert L.sc_dev_rtb_expand_f64(h, d_u, nvec, nr, p(rtb._P), p(rtb._boa), p(rtb._offset), n_atoms, p(out)) == 1
    hb = torch.zeros((rtb.nr, rtb.nr), dtype=torch.float64, device=rtb.device)
    args = [h, p(rtb._coord), 21, p(rtb._pairs), rtb.n_pairs, p(rtb._gamma), None, p(rtb._P), p(rtb._boa), p(rtb._offset),
            rtb.n_blocks, rtb.nr, p(rtb._order), p(rtb._seg_start), rtb.n_segments, p(rtb._block_start), p(hb)]
    for pos, bad in [(2, 0), (4, -1), (10, 0), (11, 0), (7, None), (16, None), (12, None)]:
        a = list(args)
        a[pos] = bad
        assert L.sc_dev_rtb_hessian_f64(*a) == 1
    # k = 0 is valid and gives the zero matrix
    hb.fill_(float("nan"))
    a = list(args)
    a[3], a[4], a[5], a[12], a[13], a[14], a[15] = None, 0, None, None, None, 0, None
    assert L.sc_dev_rtb_hessian_f64(*a) == 0
    rtb.ctx.synchronize()
    assert bool((hb == 0).all())
