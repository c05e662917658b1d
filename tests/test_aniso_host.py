"""
CPU-only checks of the anisotropic fluctuation tensors (``nma.anisotropic_fluctuation``, ``nma.anisotropy``): the public
names, the errors that are raised on the host before any device call, the 6 -> 3x3 expansion with the ANISOU ordering, the
anisotropy ratio against ``np.linalg.eigvalsh``, and header against binding for the three C entries, the way
tests/test_abi_and_host.py checks the whole ABI.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_aniso", "sc_dev_modes_aniso_f64", "sc_batch_plan_modes_aniso_f64"}


def test_public_names():
    import springcraft_amd as sc
    from springcraft_amd import nma

    assert "anisotropic_fluctuation" in nma.__all__ and "anisotropy" in nma.__all__
    assert sc.nma.anisotropic_fluctuation is nma.anisotropic_fluctuation
    assert callable(sc.ANM.anisotropic_fluctuation)
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    assert callable(DeviceBatchSolver.anisotropic_fluctuation) and callable(RaggedBatchSolver.anisotropic_fluctuation)


def test_errors_are_raised_on_the_host(monkeypatch):
    """A GNM, a non-model and a trivial mode index raise before the library or a device is touched."""
    import springcraft_amd as sc
    from springcraft_amd import _hip, nma

    def no_device(*a, **k):
        raise AssertionError("the check must not reach the native library")

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)
    coord = np.random.RandomState(0).rand(10, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    for not_an_anm in (sc.GNM(coord, ff), np.eye(30), None):
        with pytest.raises(ValueError, match=r"^Instance of ANM class expected\.$"):
            nma.anisotropic_fluctuation(not_an_anm)
    anm = sc.ANM(coord, ff)
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.anisotropic_fluctuation(anm, mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            anm.anisotropic_fluctuation(mode_subset=subset)


def test_expansion_is_symmetric_in_anisou_order():
    from springcraft_amd.nma import ANISOU_INDEX, _aniso_full

    # PDB ANISOU columns: U(1,1) U(2,2) U(3,3) U(1,2) U(1,3) U(2,3)
    u6 = np.array([11.0, 22.0, 33.0, 12.0, 13.0, 23.0])
    full = _aniso_full(u6)
    assert np.array_equal(full, [[11.0, 12.0, 13.0], [12.0, 22.0, 23.0], [13.0, 23.0, 33.0]])
    assert np.array_equal(ANISOU_INDEX, ANISOU_INDEX.T) and sorted(set(ANISOU_INDEX.ravel())) == list(range(6))
    batch = np.random.RandomState(1).randn(4, 7, 6)
    full = _aniso_full(batch)
    assert full.shape == (4, 7, 3, 3)
    assert np.array_equal(full, full.swapaxes(-1, -2))
    assert np.array_equal(np.trace(full, axis1=-2, axis2=-1), batch[..., :3].sum(axis=-1))
    for e, (d0, d1) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        assert np.array_equal(full[..., d0, d1], batch[..., e])
    # the same gather is what the batch solvers enqueue on the device (torch.index_select with the flattened indices)
    import torch

    t = torch.from_numpy(batch).index_select(-1, torch.from_numpy(ANISOU_INDEX.reshape(-1))).view(4, 7, 3, 3)
    assert np.array_equal(t.numpy(), full)


def test_anisotropy_against_eigvalsh():
    from springcraft_amd.nma import anisotropy

    rs = np.random.RandomState(2)
    a = rs.randn(3, 25, 3, 3)
    spd = a @ a.swapaxes(-1, -2) + 1e-3 * np.eye(3)
    lam = np.linalg.eigvalsh(spd)
    got = anisotropy(spd)
    assert got.shape == (3, 25)
    assert np.allclose(got, lam[..., 0] / lam[..., 2])
    assert np.all((got > 0) & (got <= 1))
    assert np.allclose(anisotropy(2.5 * np.eye(3)[None]), [1.0])
    # a zero tensor (an empty selection) and a NaN tensor (a failed structure): NaN, and no warning from the division
    mixed = np.stack([np.zeros((3, 3)), spd[0, 0], np.full((3, 3), np.nan)])
    with np.errstate(all="raise"):
        got = anisotropy(mixed)
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == pytest.approx(lam[0, 0, 0] / lam[0, 0, 2])
    with pytest.raises(ValueError):
        anisotropy(np.zeros((4, 6)))


def test_header_declares_the_three_entries_and_the_binding_names_exactly_those():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "aniso" in n}
    assert declared == ENTRIES
    assert {n for n in _hip.EXPORTED_SYMBOLS if "aniso" in n} == ENTRIES
    proto = {
        "sc_modes_aniso": r"int sc_modes_aniso\(sc_modes\* modes, const int64_t\* mode_idx, int64_t k, double\* out\);",
        "sc_dev_modes_aniso_f64": r"int sc_dev_modes_aniso_f64\(sc_ctx\* ctx, const double\* d_w, const double\* d_v, "
                                  r"int64_t m, int64_t nvec, int64_t batch,\s+const sc_mode_selection\* sel, "
                                  r"const int64_t\* d_counts, double\* d_out\);",
        "sc_batch_plan_modes_aniso_f64": r"int sc_batch_plan_modes_aniso_f64\(sc_batch_plan\* plan, const double\* d_w, "
                                         r"const double\* d_v, int64_t nvec,\s+const sc_mode_selection\* sel, "
                                         r"const int64_t\* d_counts, double\* d_out\);",
    }
    for name, pat in proto.items():
        assert re.search(pat, header), name
    L = _hip.lib()
    nargs = {"sc_modes_aniso": 4, "sc_dev_modes_aniso_f64": 9, "sc_batch_plan_modes_aniso_f64": 7}
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs[name], name
    assert callable(_hip.Modes.aniso)
    # the workspace queries answer for what = 2 (ANM shapes only) without a device
    assert L.sc_dev_modes_workspace_bytes(513, 513, 3, 3, 507, 2, 0) > 0
    assert L.sc_dev_modes_workspace_bytes(513, 513, 3, 1, 507, 2, 0) == 0
    assert L.sc_dev_modes_workspace_bytes(512, 512, 3, 3, 506, 2, 0) == 0
