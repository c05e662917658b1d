"""
CPU checks of the batched subsystem reduction on a common core (:class:`springcraft_amd.SubsystemBatch`): the host helper
``aligned_core``, the argument refusals that need no device, the facts about the members that
tests/test_subsystem_batch_gpu.py relies on, the property the device design rests on (a slot ``diag(H_ee, I)`` with zero pad
rows of H_es reduces to the SAME H_eff), the specification's own float64 error against its longdouble evaluation (the pinned
gates), the C ABI's declarations, and the pure host logic of csrc/potrf_policy.h under sanitizers.
"""
import shutil
import subprocess
from os.path import dirname, join

import numpy as np
import pytest

from tests import subsystem_batch_model as bm
from tests import subsystem_model as sm

ROOT = dirname(dirname(__file__))
MEMBER_IDS = range(len(bm.MEMBERS))


# ---- aligned_core ------------------------------------------------------------------------------------------------------------
def test_aligned_core_keeps_the_gap_free_columns_in_order():
    from springcraft_amd import aligned_core

    alignment = np.array([[0, 1, -1, 2, 3, 4, -1],
                          [5, -1, 0, 4, 1, 2, 3],
                          [-1, 0, 1, 9, 3, 2, 4]])
    columns, systems = aligned_core(alignment)
    assert columns.tolist() == [3, 4, 5] and columns.dtype == np.int64
    assert [s.tolist() for s in systems] == [[2, 3, 4], [4, 1, 2], [9, 3, 2]]   # the column order, not ascending
    assert all(s.dtype == np.int64 and s.flags.c_contiguous for s in systems)
    columns, systems = aligned_core([[3, 1, 2]])                                 # one member, no gap
    assert columns.tolist() == [0, 1, 2] and systems[0].tolist() == [3, 1, 2]
    # the result is what SubsystemBatch takes: every system passes subsystem_partition on a structure that has a gap atom
    from springcraft_amd import subsystem_partition

    for s in aligned_core(alignment)[1]:
        assert subsystem_partition(10, s)[0].tolist() == s.tolist()


@pytest.mark.parametrize("bad, message", [
    ([[0, 1, 1], [0, 1, 2]], "member 0.*twice"), ([[0, 1, 2], [2, -1, 2]], "member 1.*twice"), ([[0, -2, 1]], "below -1"),
    ([[0, -1], [-1, 0]], "no gap-free column"), ([[-1, -1]], "no gap-free column"), ([0, 1, 2], "shape"),
    ([[0.0, 1.0]], "integer"), (np.zeros((0, 3), dtype=int), "shape"), (np.zeros((2, 0), dtype=int), "no gap-free column"),
])
def test_aligned_core_refusals(bad, message):
    from springcraft_amd import aligned_core

    with pytest.raises(ValueError, match=message):
        aligned_core(np.asarray(bad))


# ---- refusals of SubsystemBatch that need no device ----------------------------------------------------------------------------
def test_refusals_without_a_device():
    import springcraft_amd as sc

    ff = sc.InvariantForceField(sm.CUTOFF)
    c = [np.array(bm.member_inputs(i)[0]) for i in (1, 2)]
    s = [bm.member_inputs(i)[1] for i in (1, 2)]
    with pytest.raises(ValueError, match="one length"):
        sc.SubsystemBatch(c, ff, s[:1])
    with pytest.raises(ValueError, match="one length"):
        sc.SubsystemBatch(c, [ff], s)
    with pytest.raises(ValueError, match="at least one member"):
        sc.SubsystemBatch([], ff, [])
    with pytest.raises(ValueError, match="member 1: its system has 11 atoms"):
        sc.SubsystemBatch(c, ff, [s[0], s[1][:11]])
    with pytest.raises(ValueError, match="member 1.*twice"):
        sc.SubsystemBatch(c, ff, [s[0], np.r_[s[1][:11], s[1][0]]])
    with pytest.raises(ValueError, match="member 0.*outside"):
        sc.SubsystemBatch(c, ff, [np.r_[s[0][:11], 13], s[1]])
    with pytest.raises(ValueError, match="member 1.*built for"):
        sc.SubsystemBatch(c, [ff, _bound(sc, 7)], s)
    with pytest.raises(ValueError, match="dim"):
        sc.SubsystemBatch(c, ff, s, dim=2)
    with pytest.raises(ValueError, match="fit=True needs at least 3"):
        sc.SubsystemBatch(c, ff, [s[0][:2], s[1][:2]])
    with pytest.raises(ValueError, match="env_order = 20 is below the 21 environment atoms of member 1"):
        sc.SubsystemBatch(c, ff, s, env_order=20)
    with pytest.raises(ValueError, match="mass entries"):
        sc.SubsystemBatch(c, ff, s, masses=[None])
    # a single Subsystem still refuses the empty environment: the batch's allowance did not change the public function
    with pytest.raises(ValueError, match="use ANM"):
        sc.subsystem_partition(12, bm.member_inputs(0)[1])


def _bound(sc, natoms):
    """A force field bound to `natoms` atoms."""
    class Bound(sc.InvariantForceField):
        @property
        def natoms(self):
            return natoms

    return Bound(sm.CUTOFF)


# ---- the members ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", MEMBER_IDS)
def test_members_are_what_the_gpu_tests_assume(index):
    coord, system, ff = bm.member_inputs(index)
    rec = bm.member_spec(index)
    n = len(coord)
    assert n == (12, 13, 33, 34, 56)[index] and len(system) == bm.N_S and len(rec["e"]) == bm.N_ENV[index]
    assert 3 * len(rec["e"]) == (0, 3, 63, 66, 132)[index] and bm.ENV_ORDER == 44
    assert not np.array_equal(system, np.sort(system))             # the alignment's order, not ascending
    h = rec["h"]
    if len(rec["e"]):
        hss, hes, hee = sm.blocks(h, rec["s"], rec["e"], 3)
        lam = np.linalg.eigvalsh(hee)
        assert lam[0] >= 0.5 and lam[-1] / lam[0] <= 500         # connected: no environment atom or part moves freely
        assert np.abs(hes).max() > 0                               # coupled
        contacts = (np.abs(h.reshape(n, 3, n, 3)).sum(axis=(1, 3)) > 0).sum(axis=1) - 1
        assert contacts[rec["e"]].min() >= 1
    w = rec["w"]
    assert np.abs(w[:6]).max() <= 1e-12 * w[-1] and w[6] >= 3e-4 * w[-1]


# ---- the property the device design rests on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_order", [bm.ENV_ORDER, bm.ENV_ORDER + 5])
@pytest.mark.parametrize("index", MEMBER_IDS)
def test_the_pad_contributes_exact_zeros(index, env_order):
    rec = bm.member_spec(index)
    own = 3 * len(rec["e"])
    for dtype in (np.float64, np.longdouble):
        h = rec["h"].astype(dtype)
        heff, l, y = bm.effective_hessian(h, rec["s"], rec["e"], 3)
        peff, pl, py = bm.padded_effective_hessian(h, rec["s"], rec["e"], 3, env_order)
        # the factor of the slot is diag(L_b, I) and Y's pad rows are 0, exactly, in either precision
        assert np.array_equal(pl[own:, own:], np.eye(3 * env_order - own))
        assert not pl[own:, :own].any() and not pl[:own, own:].any() and not py[own:].any()
        top = np.abs(heff).max()
        xs = np.random.RandomState(index).randn(3, len(heff))
        full = sm.follow(pl, py, xs)
        assert not full[:, own:].any()                             # the pad does not move
        if dtype is np.longdouble:
            # NumPy sums longdouble products in sequence: the pad's exact zeros change no bit of L, Y, H_eff or x_e
            assert np.array_equal(pl[:own, :own], l) and np.array_equal(py[:own], y) and np.array_equal(peff, heff)
            if own:
                assert np.array_equal(full[:, :own], sm.follow(l, y, xs))
        else:
            # (float64 products go through BLAS, whose summation order depends on the operands' extents)
            assert np.abs(peff - heff).max() <= sm.gate(bm.pinned(index, len(heff), top), rec["n"], top)


@pytest.mark.parametrize("index", MEMBER_IDS)
def test_specification_error_is_pinned(index):
    rec = bm.member_spec(index)
    heff = rec["heff"]
    exact = bm.effective_hessian(rec["h"].astype(np.longdouble), rec["s"], rec["e"], 3)[0]
    err = float(np.abs(heff - exact).max() / (len(heff) * sm.EPS * np.abs(heff).max()))
    print(f"member {index}: |H_eff(f64) - H_eff(longdouble)| / (3 n_s eps max|H_eff|) = {err:.4f}")
    if bm.N_ENV[index] == 0:
        assert err == 0.0 and bm.SPEC_ERROR[index] == 0.0            # nothing is reduced
    else:
        assert 0.25 * bm.SPEC_ERROR[index] <= err <= bm.SPEC_ERROR[index]
    # eight times that is below the floor n eps scale: the floor governs the GPU gates
    scale = np.abs(heff).max()
    assert sm.gate(bm.pinned(index, len(heff), scale), rec["n"], scale) == rec["n"] * sm.EPS * scale


def test_fit_family_is_rigid():
    family, system = bm.fit_family()
    base = family[0]
    d0 = np.linalg.norm(base[:, None] - base[None], axis=-1)
    for c, (axis, angle, _) in zip(family[:3], bm.POSES):
        r = bm.rotation(axis, angle)
        assert abs(np.linalg.det(r) - 1.0) <= 1e-14 and np.abs(r @ r.T - np.eye(3)).max() <= 1e-14
        assert np.abs(np.linalg.norm(c[:, None] - c[None], axis=-1) - d0).max() <= 1e-12
    assert 0.5 * bm.PERTURBATION <= np.abs(family[3] - base).std() <= 2 * bm.PERTURBATION


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sc_dev_vsa_batch_workspace", "sc_dev_vsa_batch_blocks_f64", "sc_dev_vsa_batch_reduce_f64")


def test_entries_are_declared_bound_and_exported():
    import ctypes as C
    import re

    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if "vsa_batch" in n} == set(ENTRIES)
    assert {n for n in _hip.EXPORTED_SYMBOLS if "vsa_batch" in n} == set(ENTRIES)
    L = _hip.lib()
    for name in ENTRIES:
        assert getattr(L, name).argtypes is not None, name
    # the argument checks that need no context
    size = C.c_size_t(7)
    ok, bad = _hip.SC_OK, _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_vsa_batch_workspace(3, 12, 44, 5, None) == bad
    for args in ((2, 12, 44, 5), (3, 0, 44, 5), (3, 12, -1, 5), (3, 12, 44, 0), (3, 12, 44, 65536)):
        assert L.sc_dev_vsa_batch_workspace(*args, C.byref(size)) == bad, args
    assert L.sc_dev_vsa_batch_workspace(3, 12, 0, 5, C.byref(size)) == ok and size.value == 0
    assert L.sc_dev_vsa_batch_workspace(3, 12, 44, 5, C.byref(size)) == ok
    # at least the inverted diagonal blocks of both passes and the panel and substitution buffers
    assert size.value >= 8 * 5 * (2 * 3 * 64 * 64 + 132 * 64 + 36 * 64)
    one = C.c_size_t(0)
    assert L.sc_dev_vsa_batch_workspace(3, 12, 44, 1, C.byref(one)) == ok and one.value < size.value
    assert L.sc_dev_vsa_batch_blocks_f64(None, None, 1, 3, 12, 0, *[None] * 10) == bad
    assert L.sc_dev_vsa_batch_reduce_f64(None, None, None, None, 36, 0, 1, None) == bad


# ---- pure host logic (slot order, refusals, carve sizes) under sanitizers ---------------------------------------------------------------
def test_batch_policy_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_subsystem_batch_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_subsystem_batch_policy.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "subsystem batch policy ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
