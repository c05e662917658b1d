"""
CPU checks of the subsystem (VSA) feature: the NumPy specification (tests/subsystem_model.py) against ``np.linalg`` on the
oracle's matrices, the facts about the inputs that tests/test_subsystem_gpu.py relies on, the specification's own float64
error against its longdouble evaluation (the pinned gates), LAPACK's factor under the ratio the device factor is held to,
``subsystem_partition``'s refusals, the C ABI's declarations, and the pure host logic of csrc/potrf_policy.h under sanitizers.
"""
import shutil
import subprocess
from os.path import dirname, join

import numpy as np
import pytest

from tests import subsystem_model as sm

ROOT = dirname(dirname(__file__))
CASE_IDS = range(len(sm.CASES))


def spec(index, dtype=np.float64, dim=3):
    coord, system, _ = sm.case_inputs(index) if dim == 3 else sm.dim1_inputs(index)
    h = sm.oracle_matrix(index, dim).astype(dtype)
    s, e = sm.partition(len(coord), system)
    return (h, s, e) + sm.effective_hessian(h, s, e, dim)


# ---- the specification against np.linalg ------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", CASE_IDS)
def test_specification_against_numpy_solve(index):
    h, s, e, heff, l, y = spec(index)
    hss, hes, hee = sm.blocks(h, s, e, 3)
    ref = hss - hes.T @ np.linalg.solve(hee, hes)
    top = np.abs(ref).max()
    assert np.abs(heff - ref).max() <= 3 * len(h) * sm.EPS * top
    xs = np.random.RandomState(index).randn(4, len(hss))
    xe = sm.follow(l, y, xs)
    ref_e = -np.linalg.solve(hee, hes @ xs.T).T
    assert np.abs(xe - ref_e).max() <= 3 * len(h) * sm.EPS * np.abs(ref_e).max() * np.linalg.cond(hee) ** 0.5
    # the defining property: with the environment following, the full matrix acts on the system alone
    x = np.zeros((4, len(h)))
    x[:, sm.dof(s, 3)], x[:, sm.dof(e, 3)] = xs, xe
    hx = x @ h
    assert np.abs(hx[:, sm.dof(e, 3)]).max() <= len(h) * sm.EPS * np.abs(h).max() * np.abs(x).max() * 8
    assert np.abs(hx[:, sm.dof(s, 3)] - xs @ heff).max() <= len(h) * sm.EPS * np.abs(h).max() * np.abs(x).max() * 8


@pytest.mark.parametrize("index", CASE_IDS)
def test_inputs_are_what_the_gpu_tests_assume(index):
    h, s, e, heff, l, y = spec(index)
    hee = sm.blocks(h, s, e, 3)[2]
    assert len(hee) == (36, 66, 129, 210, 387)[index]
    lam = np.linalg.eigvalsh(hee)
    assert lam[0] >= 0.76 and 15 <= lam[-1] / lam[0] <= 850
    # (the oracle sums its diagonal blocks down the columns: symmetric to rounding, not bit for bit)
    assert np.abs(h - h.T).max() <= 8 * sm.EPS * np.abs(h).max()
    assert np.abs(heff - heff.T).max() <= 64 * sm.EPS * np.abs(heff).max()
    w = np.linalg.eigvalsh(0.5 * (heff + heff.T))
    assert np.abs(w[:6]).max() <= 2e-13 and w[6] >= 3.7e-4 * w[-1]


@pytest.mark.parametrize("index", range(len(sm.CASES_DIM1)))
def test_dim_1_inputs(index):
    h, s, e, heff, l, y = spec(index, dim=1)
    assert len(e) == (1, 65, 43)[index]
    w = np.linalg.eigvalsh(0.5 * (heff + heff.T))
    assert abs(w[0]) <= 2e-12 and w[1] >= 1e-2 * w[-1]
    hss, hes, hee = sm.blocks(h, s, e, 1)
    assert np.abs(heff - (hss - hes.T @ np.linalg.solve(hee, hes))).max() <= 3 * len(h) * sm.EPS * np.abs(heff).max()


def test_masses_scale_rows_and_columns():
    h, s, e, heff, _, _ = spec(0)
    t = 1.0 / np.sqrt(sm.masses_of(len(h) // 3)[s])
    scaled = sm.effective_hessian(h, s, e, 3, t)[0]
    tt = np.repeat(t, 3)
    assert np.abs(scaled - heff * tt[:, None] * tt[None, :]).max() <= 8 * sm.EPS * np.abs(scaled).max()


# ---- the pinned error of the specification, and LAPACK under the device's ratio ------------------------------------------------------
@pytest.mark.parametrize("index", CASE_IDS)
def test_specification_error_is_pinned(index):
    heff = spec(index)[3]
    exact = spec(index, np.longdouble)[3]
    err = float(np.abs(heff - exact).max() / (len(heff) * sm.EPS * np.abs(heff).max()))
    print(f"case {index}: |H_eff(f64) - H_eff(longdouble)| / (3 n_s eps max|H_eff|) = {err:.4f}")
    assert 0.25 * sm.SPEC_ERROR[index] <= err <= sm.SPEC_ERROR[index]
    # eight times that is far below the floor n eps scale: the floor governs the GPU gates
    n = 3 * sm.CASES[index][0]
    scale = np.abs(heff).max()
    assert sm.gate(sm.SPEC_ERROR[index] * len(heff) * sm.EPS * scale, n, scale) == n * sm.EPS * scale


@pytest.mark.parametrize("index", CASE_IDS)
def test_unblocked_factor_ratio(index):
    h, s, e, heff, l, y = spec(index)
    hee = sm.blocks(h, s, e, 3)[2]
    assert sm.factor_ratio(hee, l) <= 0.024
    assert sm.factor_ratio(hee, np.linalg.cholesky(hee)) <= 5.0


@pytest.mark.parametrize("cond", sm.POTRF_CONDS)
@pytest.mark.parametrize("n", sm.POTRF_ORDERS)
def test_lapack_factor_ratio_on_the_potrf_inputs(n, cond):
    a = sm.spd(n, cond)
    assert np.array_equal(a, a.T)
    if n > 1:
        assert 0.5 * cond <= np.linalg.cond(a) <= 2 * cond
    l = np.linalg.cholesky(a)
    assert sm.factor_ratio(a, l) <= 5.0
    if n <= 200:
        own = sm.cholesky(a)
        assert sm.factor_ratio(a, own) <= 5.0
        b = np.random.RandomState(n).randn(n, 5)
        y = sm.forward(own, b)
        x = sm.backward(own, y)
        assert sm.triangular_ratio(own, y, b) <= 5.0 and sm.triangular_ratio(own.T, x, y) <= 5.0
        assert sm.solve_ratio(a, x, b) <= 5.0


def test_specification_refuses_an_indefinite_matrix():
    a = np.array(sm.spd(17, 1e6))
    a[9, 9] -= 2 * np.linalg.cholesky(a)[9, 9] ** 2
    assert sm.cholesky(a) is None and sm.cholesky(sm.spd(17, 1e6)) is not None


# ---- the product's host function -------------------------------------------------------------------------------------------------
def test_subsystem_partition():
    from springcraft_amd import subsystem_partition

    s, e, group, pos = subsystem_partition(6, [4, 1, 3])
    assert s.tolist() == [4, 1, 3] and e.tolist() == [0, 2, 5] and s.dtype == e.dtype == np.int64
    assert group.tolist() == [1, 0, 1, 0, 0, 1] and group.dtype == np.int32
    assert pos.tolist() == [0, 1, 1, 2, 0, 2] and pos.dtype == np.int32
    mask = np.array([False, True, False, True, True, False])
    s, e, group2, pos2 = subsystem_partition(6, mask)
    assert s.tolist() == [1, 3, 4] and e.tolist() == [0, 2, 5] and group2.tolist() == group.tolist()
    assert pos2.tolist() == [0, 0, 1, 1, 2, 2]
    for index in CASE_IDS:
        coord, system, _ = sm.case_inputs(index)
        got = subsystem_partition(len(coord), system)
        ref = sm.partition(len(coord), system)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("bad, message", [
    ([0, 0, 1], "twice"), ([0, 6], "outside"), ([-1, 2], "outside"), ([], "empty"), (np.zeros(6, dtype=bool), "empty"),
    (np.zeros(5, dtype=bool), "mask of shape"), ([0.5, 1.0], "integer"), ([[0, 1]], "shape"),
    (np.arange(6), "use ANM"), (np.ones(6, dtype=bool), "use ANM"),
])
def test_subsystem_partition_refusals(bad, message):
    from springcraft_amd import subsystem_partition

    with pytest.raises(ValueError, match=message):
        subsystem_partition(6, np.asarray(bad))
    with pytest.raises(ValueError, match="positive"):
        subsystem_partition(0, [0])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sc_dev_potrf_workspace", "sc_dev_potrf_f64", "sc_dev_potrs_f64", "sc_dev_subsystem_blocks_f64",
           "sc_dev_subsystem_reduce_f64", "sc_dev_subsystem_follow_f64")


def test_entries_are_declared_bound_and_exported():
    import re

    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    assert {n for n in _hip.EXPORTED_SYMBOLS if "potr" in n or "subsystem" in n} == set(ENTRIES) <= declared
    L = _hip.lib()
    for name in ENTRIES:
        assert getattr(L, name).argtypes is not None
    # the argument checks that need no context
    import ctypes as C

    size = C.c_size_t(0)
    assert L.sc_dev_potrf_workspace(0, 1, C.byref(size)) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_potrf_workspace(64, 1, None) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_potrf_workspace(64, 1, C.byref(size)) == _hip.SC_OK and size.value >= 2 * 64 * 64 * 8
    assert L.sc_dev_potrf_f64(None, None, 4, 4, 16, 1, None) == _hip.SC_ERR_INVALID_ARG


def test_product_code_does_not_call_torch_cholesky():
    import glob

    for path in glob.glob(join(ROOT, "springcraft_amd", "*.py")):
        assert "linalg.cholesky" not in open(path).read(), path


# ---- pure host logic (block plan, substitution steps, scratch layouts) under sanitizers ----------------------------------------------
def test_potrf_policy_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_potrf_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_potrf_policy.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "potrf policy ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
