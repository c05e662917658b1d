"""
CPU-only checks of the mode overlaps and collectivities (``nma.overlap``, ``nma.collectivity``,
``nma.cumulative_overlap``): the public names, the errors that are raised on the host before the library or a device is
touched, the cumulative overlap against its NumPy expression (NumPy and torch input, completeness over an orthogonal
basis), and header against binding for the three C entries, the way tests/test_abi_and_host.py checks the whole ABI.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_overlap", "sc_dev_modes_overlap_f64", "sc_batch_plan_modes_overlap_f64"}


def test_public_names():
    import springcraft_amd as sc
    from springcraft_amd import nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    for name in ("overlap", "collectivity", "cumulative_overlap"):
        assert name in nma.__all__ and callable(getattr(sc.nma, name))
    for cls in (sc.ANM, sc.GNM, DeviceBatchSolver, RaggedBatchSolver):
        assert callable(cls.overlap) and callable(cls.collectivity)
    for fn in (nma.overlap, nma.collectivity, nma.cumulative_overlap, DeviceBatchSolver.overlap,
               DeviceBatchSolver.collectivity):
        assert "no reference counterpart" in fn.__doc__.lower()
    assert "sqrt(mass)" in nma.overlap.__doc__ and "sqrt(mass)" in DeviceBatchSolver.overlap.__doc__


def test_errors_are_raised_on_the_host(monkeypatch):
    """A wrong model, a wrong displacement shape and a trivial mode index raise before the library or a device is touched."""
    import springcraft_amd as sc
    from springcraft_amd import _hip, nma

    def no_device(*a, **k):
        raise AssertionError("the check must not reach the native library")

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)
    n = 10
    coord = np.random.RandomState(0).rand(n, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    anm, gnm = sc.ANM(coord, ff), sc.GNM(coord, ff)
    for not_a_model in (np.eye(30), None):
        with pytest.raises(ValueError, match="Instance of GNM/ANM class expected"):
            nma.overlap(not_a_model, np.zeros((n, 3)))
        with pytest.raises(ValueError, match="Instance of GNM/ANM class expected"):
            nma.collectivity(not_a_model)
    for bad in (np.zeros((n,)), np.zeros((n + 1, 3)), np.zeros((n, 2)), np.zeros((2, n + 1, 3)), np.zeros((3 * n,)),
                np.zeros((2, 2, n, 3)), 1.0):
        with pytest.raises(ValueError, match=r"\(N, 3\) or \(q, N, 3\) with N = 10"):
            nma.overlap(anm, bad)
        with pytest.raises(ValueError, match=r"\(N, 3\) or \(q, N, 3\) with N = 10"):
            anm.overlap(bad)
    for bad in (np.zeros((n, 3)), np.zeros((n + 1,)), np.zeros((2, n + 1)), np.zeros((2, 2, n))):
        with pytest.raises(ValueError, match=r"\(N,\) or \(q, N\) with N = 10"):
            nma.overlap(gnm, bad)
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.overlap(anm, np.ones((n, 3)), mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            anm.collectivity(mode_subset=subset)
    with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
        gnm.overlap(np.ones(n), mode_subset=[0, 3])
    with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
        nma.collectivity(gnm, mode_subset=[0])


def test_cumulative_overlap_numpy_and_torch():
    import torch

    from springcraft_amd.nma import cumulative_overlap

    rs = np.random.RandomState(3)
    o = rs.uniform(-1, 1, (4, 3, 17))
    ref = np.sqrt(np.cumsum(o**2, -1))
    got = cumulative_overlap(o)
    assert isinstance(got, np.ndarray) and got.shape == o.shape and np.allclose(got, ref, rtol=1e-14, atol=0)
    assert np.allclose(cumulative_overlap(o[0, 0]), ref[0, 0], rtol=1e-14, atol=0)
    assert np.allclose(cumulative_overlap(o[0, 0].tolist()), ref[0, 0], rtol=1e-14, atol=0)
    t = cumulative_overlap(torch.from_numpy(o))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == o.shape
    assert np.allclose(t.numpy(), ref, rtol=1e-14, atol=0)
    assert np.all(np.diff(got, axis=-1) >= 0)
    # the rows of an orthogonal matrix as modes: a complete orthonormal basis, the cumulative overlap ends at 1
    q_mat, _ = np.linalg.qr(rs.randn(30, 30))
    modes = q_mat.T
    d = rs.randn(5, 30)
    ov = (d @ modes.T) / (np.linalg.norm(d, axis=1)[:, None] * np.linalg.norm(modes, axis=1)[None, :])
    assert np.allclose(cumulative_overlap(ov)[:, -1], 1.0, rtol=1e-12, atol=0)
    assert np.allclose(cumulative_overlap(torch.from_numpy(ov))[:, -1].numpy(), 1.0, rtol=1e-12, atol=0)


def test_header_declares_the_three_entries_and_the_binding_binds_them():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "overlap" in n}
    assert declared == ENTRIES
    assert {n for n in _hip.EXPORTED_SYMBOLS if "overlap" in n} == ENTRIES
    assert not any("aniso" in n for n in ENTRIES)
    proto = {
        "sc_dev_modes_overlap_f64":
            r"int sc_dev_modes_overlap_f64\(sc_ctx\* ctx, const double\* d_v, int64_t m, int64_t nvec, int64_t batch, "
            r"int dim,\s+const double\* d_disp, int64_t q, const int64_t\* d_counts, double\* d_overlap,\s+"
            r"double\* d_collectivity\);",
        "sc_batch_plan_modes_overlap_f64":
            r"int sc_batch_plan_modes_overlap_f64\(sc_batch_plan\* plan, const double\* d_v, int64_t nvec, "
            r"int64_t first_row,\s+const double\* d_disp, int64_t q, const int64_t\* d_counts, double\* d_overlap,\s+"
            r"double\* d_collectivity\);",
        "sc_modes_overlap":
            r"int sc_modes_overlap\(sc_modes\* modes, const int64_t\* mode_idx, int64_t k, const double\* disp, "
            r"int64_t q,\s+double\* overlap_out, double\* collectivity_out\);",
    }
    for name, pat in proto.items():
        assert re.search(pat, header), name
    L = _hip.lib()
    nargs = {"sc_dev_modes_overlap_f64": 11, "sc_batch_plan_modes_overlap_f64": 9, "sc_modes_overlap": 7}
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs[name], name
    assert callable(_hip.Modes.overlap)
    # no workspace: what = 3 answers 0 for shapes at which the other consumers answer a size
    assert L.sc_dev_modes_workspace_bytes(513, 513, 3, 3, 507, 0, 0) > 0
    assert L.sc_dev_modes_workspace_bytes(513, 513, 3, 3, 507, 3, 0) == 0
    assert L.sc_dev_modes_workspace_bytes(512, 512, 3, 1, 511, 3, 0) == 0
