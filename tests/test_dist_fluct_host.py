"""
CPU-only checks of the distance fluctuations (``csrc/dist_fluct.hip`` behind ``sc_dev_modes_distfluct_f64``,
``sc_batch_plan_modes_distfluct_f64`` and ``sc_modes_distfluct``): the public names, the three C entries in the header,
the symbol table and the ctypes table, the workspace answer for ``what = 4``, the host-side argument errors (raised before
any device call), ``nma.effective_stiffness`` and the NumPy model that tests/test_dist_fluct_gpu.py uses as its oracle.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))
ENTRIES = ("sc_modes_distfluct", "sc_dev_modes_distfluct_f64", "sc_batch_plan_modes_distfluct_f64")


# ---- the model: the definition, evaluated directly ---------------------------------------------------------------------
def np_distfluct(w, v, rows, coord, scale=None):
    """
    F[a, c] = sum_{r in rows} (n_ac . (u_r[c] - u_r[a]))^2 / w_r on (w (k,), v (k, >= 3N) rows = modes, coord (N, 3)), u =
    scale[:, None] * v; float64, row by row in the order of ``rows``.  The diagonal is 0; two atoms at one position: NaN.
    """
    rows = np.asarray(rows, dtype=np.int64)
    coord = np.asarray(coord, dtype=np.float64)
    n_atoms = len(coord)
    d = coord[None, :, :] - coord[:, None, :]                    # d[a, c] = x_c - x_a
    with np.errstate(invalid="ignore", divide="ignore"):
        n = d / np.sqrt((d * d).sum(axis=-1))[:, :, None]
    nx, ny, nz = (np.ascontiguousarray(n[:, :, k]) for k in range(3))      # (planes: a row costs three passes, not a gather)
    out = np.zeros((n_atoms, n_atoms))
    for r in rows:
        u = v[r, :3 * n_atoms].reshape(n_atoms, 3)
        if scale is not None:
            u = u * scale[:, None]
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        p = nx * (ux[None, :] - ux[:, None]) + ny * (uy[None, :] - uy[:, None]) + nz * (uz[None, :] - uz[:, None])
        out += p * p / w[r]
    np.fill_diagonal(out, 0.0)
    return out


def np_unprojected(w, v, rows, n_atoms, dim=3):
    """c_aa + c_cc - 2 c_ac of the unnormalised cross-correlations over ``rows``."""
    rows = np.asarray(rows, dtype=np.int64)
    u = v[rows, :dim * n_atoms].reshape(len(rows), n_atoms, dim)
    c = np.einsum("k,kad,kcd->ac", 1.0 / w[rows], u, u)
    d = np.diag(c)
    return (d[:, None] + d[None, :]) - 2 * c


def test_projected_over_three_orthogonal_directions_is_the_unprojected_form():
    """N = 12, a random orthonormal basis as modes: per pair, n and two directions orthogonal to it span the space."""
    rs = np.random.RandomState(3)
    n_atoms = 12
    m = 3 * n_atoms
    v = np.linalg.qr(rs.randn(m, m))[0].T.copy()
    w = rs.uniform(0.5, 20.0, m)
    coord = rs.rand(n_atoms, 3) * 10.0
    rows = np.arange(6, m)
    total = np.zeros((n_atoms, n_atoms))
    d = coord[None, :, :] - coord[:, None, :]
    for a in range(n_atoms):
        for c in range(n_atoms):
            if a == c:
                continue
            # an orthonormal frame whose first vector is n_ac
            frame = np.linalg.qr(np.column_stack([d[a, c], rs.randn(3), rs.randn(3)]))[0]
            for k in range(3):
                u = v[rows].reshape(len(rows), n_atoms, 3)
                p = (u[:, c] - u[:, a]) @ frame[:, k]
                total[a, c] += (p * p / w[rows]).sum()
    ref = np_unprojected(w, v, rows, n_atoms)
    off = ~np.eye(n_atoms, dtype=bool)
    assert np.allclose(total[off], ref[off], rtol=1e-12, atol=0)
    # and the first direction alone is the projected definition
    first = np_distfluct(w, v, rows, coord)
    assert np.all(first <= ref * (1 + 1e-12)) and np.all(first >= 0) and np.array_equal(first, first.T)
    assert not np.any(np.diag(first))


# ---- names -----------------------------------------------------------------------------------------------------------------
def test_public_names_and_docstrings():
    import springcraft_amd as sc
    from springcraft_amd import nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    assert "distance_fluctuation" in nma.__all__ and "effective_stiffness" in nma.__all__
    owners = [nma.distance_fluctuation, DeviceBatchSolver.distance_fluctuation, RaggedBatchSolver.distance_fluctuation]
    for fn in owners:
        doc = fn.__doc__
        assert "no reference counterpart" in doc.lower(), fn
        assert "inv_sqrt_mass" in doc, fn
    for fn in (sc.ANM.distance_fluctuation, sc.GNM.distance_fluctuation, nma.effective_stiffness):
        assert "no reference counterpart" in fn.__doc__.lower(), fn


def _declaration(header, name):
    mt = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert mt, name
    return [a.strip() for a in mt.group(1).split(",")]


def test_header_symbol_table_and_argtypes_agree():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    L = _hip.lib()
    expected = {"sc_modes_distfluct": 5, "sc_dev_modes_distfluct_f64": 11, "sc_batch_plan_modes_distfluct_f64": 9}
    for name in ENTRIES:
        args = _declaration(header, name)
        assert name in _hip.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert len(args) == len(fn.argtypes) == expected[name], (name, args, fn.argtypes)
        assert "overlap" not in name and "aniso" not in name
        # the comment in front of the declaration says where it comes from
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "no reference counterpart" in comment.lower() and "calcDistFlucts" in comment and "calcMechStiff" in comment, name
    assert _declaration(header, "sc_dev_modes_distfluct_f64")[-1].startswith("double* d_out")
    assert _declaration(header, "sc_modes_distfluct")[3].startswith("const double* coord")


# Figures of the parent commit at (m, nvec, batch, dim, n_sel) = (513, 513, 3, 3, 507), from its formulas:
# what = 1: weights 3 * 507 * 8 -> 12288, P and S of a slab of 3 structures (stride 507 * 513 -> 260096 doubles: 2 x
#           6242304), diagonals 3 * 171 * 8 -> 4352, 3 GEMM records -> 512, + 1024
# what = 2: weights 12288, partial sums 3 structures x 47 chunks (of 11 rows) x 6 x 171 x 8 -> 1157376, + 1024
PARENT_WHAT_1 = 12288 + 2 * 6242304 + 4352 + 512 + 1024
PARENT_WHAT_2 = 12288 + 1157376 + 1024


def test_workspace_code_4():
    from springcraft_amd import _hip

    ws = _hip.lib().sc_dev_modes_workspace_bytes
    assert ws(513, 513, 3, 3, 507, 4, 0) > 0
    # the weights (batch, n_sel) alone: no partial sums, nothing per atom pair
    assert ws(513, 513, 3, 3, 507, 4, 0) == (3 * 507 * 8 + 255) // 256 * 256 + 1024
    assert ws(513, 513, 3, 1, 507, 4, 0) == 0          # dim 1
    assert ws(512, 512, 3, 3, 506, 4, 0) == 0          # m % 3 != 0
    # the other codes answer what they did before (figures of the parent commit at these arguments)
    assert ws(513, 513, 3, 3, 507, 1, 0) == PARENT_WHAT_1
    assert ws(513, 513, 3, 3, 507, 2, 0) == PARENT_WHAT_2
    assert ws(513, 513, 3, 3, 507, 3, 0) == 0


# ---- argument errors come from the host ---------------------------------------------------------------------------------
def test_value_errors_are_raised_before_any_device_call(monkeypatch):
    import springcraft_amd as sc
    from springcraft_amd import _hip, nma

    def boom(*a, **k):
        raise AssertionError("the device was asked")

    monkeypatch.setattr(_hip, "lib", boom)
    monkeypatch.setattr(_hip, "context", boom)
    coord = np.random.RandomState(0).rand(10, 3) * 8.0
    ff = sc.InvariantForceField(9.0)
    with pytest.raises(ValueError, match="GNM/ANM"):
        nma.distance_fluctuation(coord)
    with pytest.raises(ValueError, match="projected"):
        nma.distance_fluctuation(sc.GNM(coord, ff))
    with pytest.raises(ValueError, match="projected"):
        sc.GNM(coord, ff).distance_fluctuation(mode_subset=[3, 4])
    with pytest.raises(ValueError, match="Trivial modes"):
        nma.distance_fluctuation(sc.ANM(coord, ff), mode_subset=[5, 7])
    with pytest.raises(ValueError, match="Trivial modes"):
        sc.ANM(coord, ff).distance_fluctuation(mode_subset=[5, 7], projected=False)
    with pytest.raises(ValueError, match="Trivial modes"):
        sc.GNM(coord, ff).distance_fluctuation(mode_subset=[0, 2], projected=False)


# ---- effective stiffness ------------------------------------------------------------------------------------------------------
def test_effective_stiffness_numpy_and_torch():
    import torch

    from springcraft_amd import nma

    f = np.array([[0.0, 0.25, np.nan], [0.25, 0.0, 4.0], [np.nan, 4.0, 0.0]])
    ref = np.array([[0.0, 4.0, np.nan], [4.0, 0.0, 0.25], [np.nan, 0.25, 0.0]])
    k = nma.effective_stiffness(f)
    assert isinstance(k, np.ndarray) and np.array_equal(k, ref, equal_nan=True)
    assert np.all(np.diag(k) == 0.0) and not np.any(np.signbit(np.diag(k)))
    kt = 300 * nma.K_B * nma.N_A
    assert np.array_equal(nma.effective_stiffness(f, tem=300, tem_factors=nma.K_B * nma.N_A), kt / np.where(f == 0, np.inf, f),
                          equal_nan=True)
    assert np.array_equal(nma.effective_stiffness(f, tem=300), (300 * nma.K_B) / np.where(f == 0, np.inf, f), equal_nan=True)
    t = torch.from_numpy(f)
    kk = nma.effective_stiffness(t)
    assert isinstance(kk, torch.Tensor) and kk.device == t.device and kk.dtype == torch.float64
    assert np.array_equal(kk.numpy(), ref, equal_nan=True)
    assert np.array_equal(nma.effective_stiffness(t, tem=300, tem_factors=nma.K_B * nma.N_A).numpy(),
                          nma.effective_stiffness(f, tem=300, tem_factors=nma.K_B * nma.N_A), equal_nan=True)
    assert np.array_equal(f, t.numpy(), equal_nan=True)        # the input is left alone
