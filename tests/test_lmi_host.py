"""
CPU-only checks of the generalized correlation (``_BatchSolver.generalized_correlation``, ``nma.generalized_correlation``):
the specification of tests/lmi_model.py against Lange & Grubmueller's 6 x 6 log-det form, its invariances, symmetry, range and
diagonal, the degenerate selections (three modes: all ones; two: all NaN), dim 1, the specification's own float64-against-
longdouble error on the GPU tests' inputs against the recorded constants, the public names, header against symbol table
against binding, the ``what = 8`` workspace answer, and the errors raised on the host before the library or a device is touched.
"""
import inspect
import re
from os.path import dirname, join

import numpy as np
import pytest

from oracle import enm_oracle as orc
from tests import lmi_model as lm
from tests.test_batch_prs_host import _fake_solver, no_device

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_lmi": 6, "sc_dev_lmi_f64": 10, "sc_batch_plan_lmi_f64": 8}


@pytest.fixture
def host_only(monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)


_CASES = {}


def lapack_case(n_atoms, masses=None):
    """LAPACK eigenpairs (rows = modes) of the oracle's Hessian of lattice(n_atoms), mass-weighted on request: once each."""
    key = (n_atoms, masses is not None)
    if key not in _CASES:
        h, _ = orc.compute_hessian(np.array(lm.lattice(n_atoms)), orc.invariant_ff(lm.CUTOFF))
        if masses is not None:
            t = np.repeat(1 / np.sqrt(masses), 3)
            h = h * t[:, None] * t[None, :]
        w, vec = np.linalg.eigh(h)
        assert np.abs(w[:6]).max() <= 1e-12 * w[-1] and w[6] >= 1e-3 * w[-1], "a disconnected network"
        _CASES[key] = (w, np.ascontiguousarray(vec.T))
    return _CASES[key]


def selections(n_atoms, w):
    out = dict(lm.subsets(n_atoms))
    out["all"] = lm.pinv_rows(w)
    return out


# ---- the specification ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", (5, 30))
def test_the_specification_is_the_log_det_formula(n_atoms):
    w, v = lapack_case(n_atoms)
    for name, rows in selections(n_atoms, w).items():
        if len(rows) < 6:
            continue                                       # (every 6 x 6 block is singular: below)
        cov = (v[rows] / w[rows][:, None]).T @ v[rows]
        r, info = lm.np_lmi(w, v, rows), lm.np_lmi(w, v, rows, information=True)
        assert np.all(np.isfinite(r))
        want_r, want_i = lm.np_lmi_logdet(cov), lm.np_lmi_logdet(cov, information=True)
        off = ~np.eye(n_atoms, dtype=bool)
        # two routes to one determinant: the error of either is eps times the condition of the 6 x 6 block, 1 / delta
        tol = 64 * lm.EPS / np.exp(-2 * want_i[off])
        assert np.all(np.abs(info[off] - want_i[off]) <= tol), (n_atoms, name)
        assert np.allclose(r[off], want_r[off], rtol=0, atol=1e-9), (n_atoms, name)
        assert np.all(np.isinf(info[~off])) and np.all(r[~off] == 1.0)
        # r = sqrt(1 - exp(-2 I / 3))
        assert np.allclose(r[off], np.sqrt(1 - np.exp(-2 * info[off] / 3)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("n_atoms", (5, 30))
def test_symmetry_range_and_diagonal(n_atoms):
    w, v = lapack_case(n_atoms)
    for name, rows in selections(n_atoms, w).items():
        r, info = lm.np_lmi(w, v, rows), lm.np_lmi(w, v, rows, information=True)
        g = lm.gate(lm.spec_error(w, v, rows), n_atoms)
        assert np.all(np.abs(r - r.T) <= g), name          # (the specification computes (a, c) and (c, a) separately)
        assert np.all((r >= 0) & (r <= 1)) and np.all(info >= 0)
        assert np.all(np.diag(r) == 1.0) and np.all(np.isposinf(np.diag(info)))


def test_invariance_under_a_scale_and_an_invertible_map_per_atom():
    n_atoms = 30
    w, v = lapack_case(n_atoms)
    rs = np.random.RandomState(7)
    scale = rs.uniform(0.2, 5.0, n_atoms)
    maps = rs.randn(n_atoms, 3, 3) + 2 * np.eye(3)
    assert np.abs(np.linalg.det(maps)).min() > 0.1
    for name, rows in selections(n_atoms, w).items():
        if len(rows) < 6:
            continue                                       # (r = 1 up to the rounding of a zero determinant)
        base = lm.np_lmi(w, v, rows)
        # the condition of the whitening enters both sides: 1e3 times the specification's own error, floor 1e-12
        tol = max(1e3 * lm.spec_error(w, v, rows), 1e-12)
        assert np.abs(lm.np_lmi(w, v, rows, scale=scale) - base).max() <= tol, name
        mapped = np.einsum("aij,kaj->kai", maps, v.reshape(len(v), n_atoms, 3)).reshape(len(v), -1)
        assert np.abs(lm.np_lmi(w, mapped, rows) - base).max() <= tol, name
    # what dcc cannot see: two atoms in lockstep along perpendicular lines.  Three modes, atom 0 moves along e_d, atom 1 along
    # e_(d+1): the trace of C_01 is 0, the generalized correlation 1
    vv = np.zeros((3, 6))
    for d in range(3):
        vv[d, d], vv[d, 3 + (d + 1) % 3] = 1.0, 1.0
    r = lm.np_lmi(np.array([1.0, 2.0, 3.0]), vv, [0, 1, 2])
    cov = (vv / np.array([1.0, 2.0, 3.0])[:, None]).T @ vv
    assert np.trace(cov[:3, 3:]) == 0.0 and np.all(r == 1.0)


@pytest.mark.parametrize("n_atoms", (5, 30, 64, 70, 130))
def test_three_modes_give_ones_and_two_give_nan(n_atoms):
    """
    Three modes: M is orthogonal and delta = 0 up to rounding.  Four and five as well -- the 6 x 6 block of a pair has rank
    k < 6 -- but there delta is one rounding-level factor times factors of order one, and its cube root shows.
    """
    w, v = lapack_case(n_atoms)
    for name in ("3", "4"):
        rows = lm.subsets(n_atoms)[name]
        r, info = lm.np_lmi(w, v, rows), lm.np_lmi(w, v, rows, information=True)
        g = lm.gate(lm.spec_error(w, v, rows), n_atoms)
        print(f"N = {n_atoms}, {name} modes: max 1 - r = {(1 - r).max():.2e}, gate {g:.2e}, min I = {info.min():.1f}")
        assert np.all(r <= 1.0) and np.all(1 - r <= g) and not np.isnan(info).any()
        assert np.all(info >= lm.info_of(1 - g))
    for k in (0, 1, 2):
        for information in (False, True):
            assert np.isnan(lm.np_lmi(w, v, np.arange(6, 6 + k), information=information)).all()
    for rows in ([6, 8], [7, 11], [9, 6]):
        assert np.isnan(lm.np_lmi(w, v, rows)).all()
    # one atom at rest in the selection: its row and column alone, the diagonal included
    still = v.copy()
    still[:, 3:6] = 0.0
    r = lm.np_lmi(w, still, lm.pinv_rows(w))
    bad = np.zeros((n_atoms, n_atoms), dtype=bool)
    bad[1, :] = bad[:, 1] = True
    assert np.array_equal(np.isnan(r), bad)
    # NaN eigenvalues: everything
    assert np.isnan(lm.np_lmi(np.full_like(w, np.nan), v, lm.pinv_rows(w))).all()


def test_dim_one_reduces_to_the_absolute_pearson_coefficient():
    rs = np.random.RandomState(11)
    a = rs.randn(12, 40)
    cov = a @ a.T / 40
    rho = cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    r = lm.np_lmi_logdet(cov, dim=1)
    off = ~np.eye(12, dtype=bool)
    assert np.allclose(r[off], np.abs(rho[off]), rtol=0, atol=1e-13)


def _measure():
    out = {}
    for n_atoms in lm.SIZES + lm.RAGGED_SIZES[:2]:
        w, v = lapack_case(n_atoms)
        for name, rows in selections(n_atoms, w).items():
            out[(n_atoms, name)] = lm.spec_error(w, v, rows)
    masses = np.random.RandomState(3).uniform(10.0, 20.0, 63)
    w, v = lapack_case(63, masses)
    out[(63, "masses")] = lm.spec_error(w, v, lm.pinv_rows(w), scale=1 / np.sqrt(masses))
    return out


def test_the_specifications_own_error_stays_within_the_recorded_constants():
    if not lm.extended():
        pytest.skip("this platform's long double is a double")
    got = _measure()
    for key, err in got.items():
        print(f"    {key!r}: {err:.1e},")
    assert set(got) == set(lm.SPEC_ERR)
    for key, err in got.items():
        assert lm.gate(err, key[0]) <= 4 * lm.gate(lm.SPEC_ERR[key], key[0]), (key, err, lm.SPEC_ERR[key])
    # r itself spans the range on these inputs
    w, v = lapack_case(130)
    r = lm.np_lmi(w, v, lm.pinv_rows(w))
    off = ~np.eye(130, dtype=bool)
    print(f"N = 130, all modes: r in [{r[off].min():.3f}, {r[off].max():.3f}]")
    assert r[off].min() > 0 and r[off].max() < 1


def test_no_block_fails_the_pivot_rule_from_four_modes_on():
    for n_atoms in lm.SIZES + lm.RAGGED_SIZES[:2]:
        w, v = lapack_case(n_atoms)
        for name, rows in selections(n_atoms, w).items():
            assert np.all(np.isfinite(lm.np_lmi(w, v, rows))), (n_atoms, name)


# ---- names, entries, workspace --------------------------------------------------------------------------------------------------
def test_public_names():
    import springcraft_amd as sc
    from springcraft_amd import batch, nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    name = "generalized_correlation"
    for cls in (DeviceBatchSolver, RaggedBatchSolver, sc.RTB, sc.EssentialDynamics):
        assert name not in vars(cls) and getattr(cls, name) is getattr(batch._BatchSolver, name)
    # no tem, no atom_scale: both cancel
    assert list(inspect.signature(batch._BatchSolver.generalized_correlation).parameters) == ["self", "mode_subset", "information"]
    assert list(inspect.signature(nma.generalized_correlation).parameters) == ["anm", "mode_subset", "information"]
    assert list(inspect.signature(sc.ANM.generalized_correlation).parameters) == ["self", "mode_subset", "information"]
    for fn in (batch._BatchSolver.generalized_correlation, nma.generalized_correlation):
        p = inspect.signature(fn).parameters
        assert p["mode_subset"].default is None and p["information"].default is False
    assert name in nma.__all__ and not hasattr(sc.GNM, name)
    s = _fake_solver(3)
    for kw in ({"tem": 300.0}, {"atom_scale": None}, {"norm": True}):
        with pytest.raises(TypeError):
            s.generalized_correlation(**kw)


def test_header_symbol_table_and_binding_name_the_three_entries():
    from springcraft_amd import _hip, batch

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "lmi" in n}
    assert declared == set(ENTRIES)
    assert {n for n in _hip.EXPORTED_SYMBOLS if "lmi" in n} == set(ENTRIES)
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name
    assert re.search(r"int sc_dev_lmi_f64\(sc_ctx\* ctx, const double\* d_w, const double\* d_v, int64_t m, int64_t nvec, "
                     r"int64_t batch,\s+const sc_mode_selection\* sel, const int64_t\* d_counts, int information, "
                     r"double\* d_out\);", header)
    assert re.search(r"int sc_modes_lmi\(sc_modes\* modes, const int64_t\* mode_idx, int64_t k, double rcond, int information, "
                     r"double\* out\);", header)
    uniform, uniform_prefix, plan, plan_prefix = batch._SCAN_ENTRIES["lmi"]
    assert (uniform, plan) == ("sc_dev_lmi_f64", "sc_batch_plan_lmi_f64")
    assert uniform_prefix == ("ctx", "w", "v", "m", "nvec", "batch") and plan_prefix == ("plan", "w", "v", "nvec")


def test_workspace_code_8():
    """The weights, the tensors' partial sums in chunks of 128 rows, the tensors (6 per atom) and the factors (9); else 0."""
    from springcraft_amd import _hip

    ws = _hip.lib().sc_dev_modes_workspace_bytes

    def up(x):
        return -(-x // 256) * 256

    m, nsel = 387, 381
    for batch in (1, 3):
        # 381 rows in chunks of 128: three partial sums of six doubles per atom
        assert ws(m, m, batch, 3, nsel, 8, 0) == (up(batch * nsel * 8) + up(batch * 3 * 6 * (m // 3) * 8) +
                                                  up(batch * (m // 3) * 6 * 8) + up(batch * (m // 3) * 9 * 8) + 1024)
    assert ws(m, m, 3, 3, nsel, 2, 0) == up(3 * nsel * 8) + up(3 * 48 * 6 * (m // 3) * 8) + 1024   # (as before: chunks of 8)
    assert ws(m, m, 3, 1, nsel, 8, 0) == 0                                    # a GNM
    assert ws(m + 1, m, 3, 3, nsel, 8, 0) == 0                                # m % 3 != 0
    # the other codes answer as before
    assert ws(m, m, 3, 3, nsel, 3, 0) == 0 and ws(m, m, 3, 3, nsel, 4, 0) == up(3 * nsel * 8) + 1024


# ---- errors raised on the host ------------------------------------------------------------------------------------------------------
def test_batch_errors_are_raised_on_the_host(host_only):
    for ragged in (False, True):
        gnm = _fake_solver(1, ragged)
        with pytest.raises(ValueError, match=r"needs an ANM solver \(dim=3\): for a GNM it is abs\(dcc\(norm=True\)\)"):
            gnm.generalized_correlation()
        novec = _fake_solver(3, ragged)
        novec.v = None
        with pytest.raises(ValueError, match="want_vectors=True"):
            novec.generalized_correlation(information=True)
    s, rag = _fake_solver(3), _fake_solver(3, ragged=True)
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        for solver in (s, rag):
            with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
                solver.generalized_correlation(subset)
    with pytest.raises(ValueError, match="mode 15 was not solved"):
        s.generalized_correlation(mode_subset=[7, 15])
    windowed = _fake_solver(3)
    windowed.window = (0.1, 2.0)
    with pytest.raises(ValueError, match="subset_by_value"):
        windowed.generalized_correlation(mode_subset=[7])


def test_one_model_errors_are_raised_on_the_host(host_only):
    import springcraft_amd as sc
    from springcraft_amd import nma

    coord = np.random.RandomState(0).rand(10, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    anm, gnm = sc.ANM(coord, ff), sc.GNM(coord, ff)
    for not_an_anm in (gnm, np.eye(30), None):
        with pytest.raises(ValueError, match=r"Instance of ANM class expected: for a GNM .* abs\(dcc\(norm=True\)\)"):
            nma.generalized_correlation(not_an_anm)
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.generalized_correlation(anm, mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            anm.generalized_correlation(subset, information=True)
    with pytest.raises(TypeError):
        nma.generalized_correlation(anm, tem=300.0)
