"""
CPU-only checks of batch perturbation-response scanning (``_BatchSolver.prs`` / ``prs_effector_sensor``, ``nma.prs`` with a
``mode_subset``): the public names, header against symbol table against binding for the three C entries, the ``what = 7``
workspace answer, the errors that are raised on the host before the library or a device is touched, the NumPy model of
tests/batch_prs.py against the reference's formula, the model in extended precision against the derived bound on the
inputs the GPU tests use (so that the gate is not one the model alone would break), and the effector / sensor profiles.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

from oracle import enm_oracle as orc
from tests.batch_prs import CUTOFF, SIZES, SUBSETS, network, np_prs, np_prs_bound, pinv_rows, ref_prs

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_prs_subset": 5, "sc_dev_prs_f64": 11, "sc_batch_plan_prs_f64": 9}


def no_device(*a, **k):
    raise AssertionError("the check must not reach the native library")


@pytest.fixture
def host_only(monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)


def _fake_solver(dim, ragged=False):
    """A batch solver's host state without a device: enough for every check that precedes the first C call."""
    import torch

    from springcraft_amd import batch as B

    if ragged:
        s = object.__new__(B.RaggedBatchSolver)
        sizes = (4, 6)
        s._layout = B._RaggedLayout(sizes, dim, [dim * n for n in sizes])
        s.batch, m = 2, dim * 6
    else:
        s = object.__new__(B.DeviceBatchSolver)
        s._layout = B._UniformLayout(3, 5, dim)
        s.batch, s.n_atoms, m = 3, 5, dim * 5
    s.torch, s.dim, s.device = torch, dim, torch.device("cuda", 0)
    s.window, s.subset, s.counts, s._first_row, s._common_modes = None, None, None, 0, m
    s.w = torch.zeros((s.batch, m), dtype=torch.float64)
    s.v = torch.zeros((s.batch, m, m), dtype=torch.float64)
    s._L, s.ctx, s._plan = None, None, None
    return s


def test_public_names():
    import inspect

    import springcraft_amd as sc
    from springcraft_amd import batch, nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    for cls in (DeviceBatchSolver, RaggedBatchSolver, sc.RTB):
        for name in ("prs", "prs_effector_sensor"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(batch._BatchSolver, name)
    assert list(inspect.signature(batch._BatchSolver.prs).parameters) == ["self", "mode_subset", "norm", "atom_scale"]
    p = inspect.signature(batch._BatchSolver.prs).parameters
    assert p["mode_subset"].default is None and p["norm"].default is True and p["atom_scale"].default is None
    assert list(inspect.signature(nma.prs).parameters) == ["anm", "norm", "mode_subset"]
    assert list(inspect.signature(sc.ANM.prs_effector_sensor).parameters) == ["self", "norm", "mode_subset"]
    assert "prs" in nma.__all__


def test_header_symbol_table_and_binding_name_the_three_entries():
    from springcraft_amd import _hip, batch

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "prs" in n}
    assert declared == set(ENTRIES) | {"sc_modes_prs"}
    assert {n for n in _hip.EXPORTED_SYMBOLS if "prs" in n} == set(ENTRIES) | {"sc_modes_prs"}
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name
    assert re.search(r"int sc_dev_prs_f64\(sc_ctx\* ctx, const double\* d_w, const double\* d_v, int64_t m, int64_t nvec, "
                     r"int64_t batch,\s+const sc_mode_selection\* sel, const int64_t\* d_counts, const double\* d_atom_scale, "
                     r"int norm,\s+double\* d_out\);", header)
    assert re.search(r"int sc_modes_prs_subset\(sc_modes\* modes, const int64_t\* mode_idx, int64_t k, int norm, double\* out\);",
                     header)
    assert callable(_hip.Modes.prs_subset)
    # the solvers' table names the two batch entries, once each in the module
    uniform, uniform_prefix, plan, plan_prefix = batch._SCAN_ENTRIES["prs"]
    assert (uniform, plan) == ("sc_dev_prs_f64", "sc_batch_plan_prs_f64")
    assert uniform_prefix == ("ctx", "w", "v", "m", "nvec", "batch") and plan_prefix == ("plan", "w", "v", "nvec")
    source = open(batch.__file__).read()
    assert source.count('"sc_dev_prs_f64"') == 1 and source.count('"sc_batch_plan_prs_f64"') == 1


def test_workspace_code_7():
    """The weights and one diagonal per structure of a slab of at most 32768; 0 where the entry refuses the shape."""
    from springcraft_amd import _hip

    ws = _hip.lib().sc_dev_modes_workspace_bytes

    def up(x):
        return -(-x // 256) * 256

    m, nsel = 387, 381
    for batch in (1, 3, 40000):
        assert ws(m, m, batch, 3, nsel, 7, 0) == up(batch * nsel * 8) + up(min(batch, 32768) * (m // 3) * 8) + 1024
    assert ws(m, m, 3, 3, 0, 7, 0) == up(3 * 8) + up(3 * 129 * 8) + 1024       # an empty selection still divides under norm
    assert ws(m, m, 3, 3, nsel, 7, 1 << 20) == ws(m, m, 3, 3, nsel, 7, 0)     # no budget: nothing is cut into slabs of bytes
    assert ws(m, m, 3, 1, nsel, 7, 0) == 0                                    # a GNM
    assert ws(m + 1, m, 3, 3, nsel, 7, 0) == 0                                # m % 3 != 0
    # the other codes answer as before
    assert ws(m, m, 3, 3, nsel, 3, 0) == 0 and ws(m, m, 3, 3, nsel, 4, 0) == up(3 * nsel * 8) + 1024


def test_batch_errors_are_raised_on_the_host(host_only):
    import torch

    for ragged in (False, True):
        gnm = _fake_solver(1, ragged)
        for call in (gnm.prs, gnm.prs_effector_sensor):
            with pytest.raises(ValueError, match="Instance of ANM class expected"):
                call()
        novec = _fake_solver(3, ragged)
        novec.v = None
        for call in (novec.prs, novec.prs_effector_sensor):
            with pytest.raises(ValueError, match="want_vectors=True"):
                call()
    s = _fake_solver(3)
    # (no test machine without a device can make a CUDA tensor: every tensor here fails the first check, as a CPU tensor)
    for bad in (torch.zeros((3, 5), dtype=torch.float64), np.zeros((3, 5)), torch.zeros((3, 5)),
                torch.zeros((5, 3), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match=r"atom_scale must be a contiguous CUDA float64 tensor of shape \(3, 5\)"):
            s.prs(atom_scale=bad)
    rag = _fake_solver(3, ragged=True)
    with pytest.raises(ValueError, match=r"atom_scale must be a contiguous CUDA float64 tensor of shape \(10,\)"):
        rag.prs_effector_sensor(atom_scale=torch.zeros(10, dtype=torch.float64))
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            s.prs(mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            rag.prs(subset, norm=False)
    with pytest.raises(ValueError, match="mode 15 was not solved"):
        s.prs(mode_subset=[7, 15])
    windowed = _fake_solver(3)
    windowed.window = (0.1, 2.0)
    with pytest.raises(ValueError, match="subset_by_value"):
        windowed.prs(mode_subset=[7])


def test_one_model_errors_are_raised_on_the_host(host_only):
    import springcraft_amd as sc
    from springcraft_amd import nma

    coord = np.random.RandomState(0).rand(10, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    anm, gnm = sc.ANM(coord, ff), sc.GNM(coord, ff)
    for not_an_anm in (gnm, np.eye(30), None):
        with pytest.raises(ValueError, match="Instance of ANM class expected"):
            nma.prs(not_an_anm, mode_subset=[7])
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.prs(anm, mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            anm.prs_effector_sensor(mode_subset=subset)
    # an assigned covariance has no modes to select from; without a subset it is reduced as before, on the host
    a = np.random.RandomState(1).randn(30, 30)
    anm.covariance = a
    with pytest.raises(ValueError, match="mode_subset cannot be combined with a covariance"):
        nma.prs(anm, mode_subset=[7, 9])
    with pytest.raises(ValueError, match="mode_subset cannot be combined with a covariance"):
        anm.prs_effector_sensor(norm=False, mode_subset=[7, 9])
    want = (a ** 2).reshape(10, 3, 10, 3).sum(axis=(1, 3))
    assert np.array_equal(nma.prs(anm, norm=False), want)
    assert np.array_equal(nma.prs(anm, True, None), want / np.diag(want)[:, None])


def test_the_model_is_the_references_formula():
    """On a random positive semi-definite 3N = 36 matrix with six null directions: np_prs over the non-trivial modes."""
    rs = np.random.RandomState(3)
    q, _ = np.linalg.qr(rs.randn(36, 36))
    lam = np.concatenate([np.zeros(6), rs.uniform(0.5, 4.0, 30)])
    h = (q * lam) @ q.T
    h = 0.5 * (h + h.T)
    w, vec = np.linalg.eigh(h)
    v = vec.T
    rows = pinv_rows(w)
    assert np.array_equal(rows, np.arange(6, 36))
    for norm in (False, True):
        got, ref = np_prs(w, v, rows, norm=norm), ref_prs(h, norm)
        assert got.shape == ref.shape == (12, 12)
        # (two routes to the same covariance, eigenvalues within a factor 8: a few hundred eps of the largest entry)
        assert np.allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    p = np_prs(w, v, rows)
    assert np.array_equal(p, p.T) or np.allclose(p, p.T, rtol=1e-14, atol=0)
    assert np.all(p >= 0)
    # a scale is the same as scaled rows, a row listed twice counts twice, no rows give zeros
    t = rs.uniform(0.5, 2.0, 12)
    assert np.allclose(np_prs(w, v, rows, scale=t), np_prs(w, v * np.repeat(t, 3)[None, :], rows), rtol=1e-13, atol=0)
    assert np.allclose(np_prs(w, v, [7, 7]), 4 * np_prs(w, v, [7]), rtol=1e-14, atol=0)
    assert not np_prs(w, v, []).any()


_CASES = {}


def lapack_case(n_atoms, seed=0):
    """LAPACK eigenpairs (rows = modes) of the oracle's Hessian of the network the GPU tests solve: once per size."""
    key = (n_atoms, seed)
    if key not in _CASES:
        h, _ = orc.compute_hessian(network(n_atoms, seed), orc.invariant_ff(CUTOFF))
        w, vec = np.linalg.eigh(h)
        assert np.abs(w[:6]).max() <= 1e-12 * w[-1] and w[6] >= 0.005 * w[-1]
        _CASES[key] = (w, np.ascontiguousarray(vec.T))
    return _CASES[key]


@pytest.mark.parametrize("n_atoms", SIZES)
def test_the_model_in_extended_precision_stays_inside_the_bound(n_atoms):
    """float64 against longdouble on the GPU tests' networks and selections: the gate is one the model itself passes."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("this platform's long double is a double")
    w, v = lapack_case(n_atoms)
    scale = 1 / np.sqrt(np.random.RandomState(3).uniform(10.0, 20.0, n_atoms))
    selections = [("pinv rule", pinv_rows(w), None), ("pinv rule, scaled", pinv_rows(w), scale)]
    if n_atoms == 20:
        selections += [(f"{k} modes", rows, None) for k, rows in SUBSETS.items()]
    else:
        selections += [("17 modes", SUBSETS[17], None), ("modes 6..25", np.arange(6, 26), scale)]
    worst = 0.0
    for name, rows, t in selections:
        exact = np_prs(w, v, rows, scale=t, dtype=np.longdouble)
        model = np_prs(w, v, rows, scale=t)
        bound = np_prs_bound(w, v, rows, t, len(rows))
        assert np.all(bound > 0)
        ratio = float((np.abs(model - exact) / bound).max())
        worst = max(worst, ratio)
        # the model's own error is half of what the bound allows between two computed values
        assert ratio <= 0.5, (n_atoms, name, ratio)
    print(f"N = {n_atoms}: float64 model against long double, max |difference| / bound = {worst:.3e}")


def test_effector_and_sensor_profiles_match_the_one_model_function():
    import torch

    from springcraft_amd import batch, nma

    rs = np.random.RandomState(5)
    p = rs.rand(3, 7, 7)
    eff, sens = batch._effector_sensor(torch, torch.from_numpy(p))
    assert tuple(eff.shape) == tuple(sens.shape) == (3, 7)
    for b in range(3):
        e, s = nma.effector_sensor(p[b])
        assert np.allclose(eff[b].numpy(), e, rtol=1e-14, atol=0) and np.allclose(sens[b].numpy(), s, rtol=1e-14, atol=0)
    one = batch._effector_sensor(torch, torch.from_numpy(p[1]))
    assert torch.equal(one[0], eff[1]) and torch.equal(one[1], sens[1])
    # NaN rows stay NaN (an empty window under norm), as in the reference's arithmetic
    nan = torch.full((2, 2), float("nan"), dtype=torch.float64)
    assert all(bool(torch.isnan(t).all()) for t in batch._effector_sensor(torch, nan))
