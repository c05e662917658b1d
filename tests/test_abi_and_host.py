"""
CPU-only checks: the C-ABI library loads and exports every symbol of include/springcraft_hip.h,
the header and the ctypes table agree, host-side logic (force fields, plans, model objects'
validation) behaves like the reference's, and the product fails loudly without a GPU.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))


def test_library_exports_every_declared_symbol():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    declared -= {"sc_ctx", "sc_ff_desc", "sc_patch_desc"}
    assert declared == set(_hip.EXPORTED_SYMBOLS)
    L = _hip.lib()
    for name in declared:
        assert hasattr(L, name), name


def test_debug_header_matches_library():
    """Every sc_dbg_* symbol the library exports is declared in include/springcraft_hip_debug.h and vice versa."""
    import subprocess
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip_debug.h")).read()
    declared = set(re.findall(r"\b(sc_dbg_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (sc_dbg_[a-z0-9_]+)$", out, re.M))
    assert declared == exported
    # and the boundary header declares everything else the library exports under the sc_ prefix
    public = set(re.findall(r"\bT (sc_[a-z0-9_]+)$", out, re.M)) - exported
    assert public == set(_hip.EXPORTED_SYMBOLS)


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import springcraft_amd as sc
    from springcraft_amd._hip import HipUnavailableError

    with pytest.raises(HipUnavailableError):
        sc.compute_kirchhoff(np.zeros((4, 3)), sc.InvariantForceField(5.0))
    with pytest.raises(HipUnavailableError):
        sc.nma.eigh(np.eye(3))


def test_product_does_not_import_oracle():
    import glob

    pat = re.compile(r"^\s*(from|import)\s+oracle\b|import_module\(.oracle|__import__\(.oracle", re.M)
    for path in glob.glob(join(ROOT, "springcraft_amd", "**", "*.py"), recursive=True):
        assert not pat.search(open(path).read()), path


def test_public_names():
    import springcraft_amd as sc

    # reference: springcraft/__init__.py:12-15 and the __all__ lists of its modules
    for name in ["GNM", "ANM", "ForceField", "PatchedForceField", "InvariantForceField",
                 "HinsenForceField", "ParameterFreeForceField", "TabulatedForceField",
                 "compute_kirchhoff", "compute_hessian"]:
        assert hasattr(sc, name)
    assert sc.__version__ == "0.3.0"


def test_force_constants_match_oracle():
    import springcraft_amd as sc
    from oracle import enm_oracle as orc

    rs = np.random.RandomState(0)
    d2 = rs.rand(1000) * 300 + 1.0
    i = np.arange(1000)
    assert np.array_equal(sc.HinsenForceField().force_constant(i, i, d2), orc.hinsen_ff().gamma(i, i, d2))
    assert np.array_equal(sc.ParameterFreeForceField().force_constant(i, i, d2), 1 / d2)
    assert np.array_equal(sc.InvariantForceField(7).force_constant(i, i, d2), np.ones(1000))


def test_device_plan():
    import springcraft_amd as sc
    from springcraft_amd.forcefield import device_plan

    d, patch, fused = device_plan(sc.InvariantForceField(7.0))
    assert fused and patch is None and d.has_cutoff == 1 and d.cutoff_sq == 49.0
    d, patch, fused = device_plan(sc.HinsenForceField())
    assert fused and d.has_cutoff == 0
    pf = sc.PatchedForceField(sc.HinsenForceField(8.0), contact_shutdown=[1])
    d, patch, fused = device_plan(pf)
    assert fused and patch[4] is True

    class Mine(sc.HinsenForceField):
        def force_constant(self, i, j, d2):
            return np.full(len(i), 2.0)

    assert device_plan(Mine(9.0))[2] is False       # subclasses may override force_constant
    nested = sc.PatchedForceField(pf, contact_shutdown=[2])
    assert device_plan(nested)[2] is False
    assert list(nested.contact_shutdown) == [2, 1]  # forcefield.py:232-239


def test_patched_force_field_host_semantics():
    """PatchedForceField.force_constant restated (forcefield.py:183-226) vs the reference-generated vectors."""
    import springcraft_amd as sc
    from tests.util import generated

    g = generated("patched_n40.npz")
    ff = sc.PatchedForceField(sc.HinsenForceField(8.0), contact_shutdown=g["shutdown"],
                              contact_pair_off=g["pair_off"], contact_pair_on=g["pair_on"],
                              force_constants=g["force_constants"])
    pairs = g["hinsen8_all_pairs"]
    coord = g["coord"]
    disp = coord[pairs[:, 1]] - coord[pairs[:, 0]]
    d2 = np.sum(disp * disp, axis=-1)
    gamma = ff.force_constant(pairs[:, 0], pairs[:, 1], d2)
    k = np.zeros((40, 40))
    k[pairs[:, 0], pairs[:, 1]] = -gamma
    np.fill_diagonal(k, -np.sum(k, axis=0))
    assert np.array_equal(k, g["hinsen8_all_kirchhoff"])


def test_tabulated_force_field_shapes():
    # reference tests: tests/test_forcefield.py:117-334 (construction rules)
    import springcraft_amd as sc

    atoms = sc.AtomArray(6)
    atoms.res_name[:] = ["ALA", "GLY", "TRP", "ALA", "TYR", "CYS"]
    atoms.chain_id[:] = ["A", "A", "A", "B", "B", "B"]
    atoms.res_id[:] = [1, 2, 3, 1, 2, 4]
    ff = sc.TabulatedForceField(atoms, 1.0, 2.0, 3.0, 10.0)
    m = ff.interaction_matrix[:, :, 0]
    assert m[0, 1] == 1.0 and m[1, 2] == 1.0 and m[3, 4] == 1.0     # bonded
    assert m[4, 5] == 2.0 and m[0, 2] == 2.0                         # same chain, not adjacent
    assert m[0, 3] == 3.0 and np.all(np.diag(m) == 0)                # other chain, self
    assert ff.natoms == 6 and ff.cutoff_distance == 10.0
    edges = np.array([4.0, 8.0, 12.0])
    ff = sc.TabulatedForceField(atoms, [1, 2, 3], [4, 5, 6], [7, 8, 9], edges)
    i = np.array([0, 0, 0]); j = np.array([3, 2, 1])
    assert list(ff.force_constant(i, j, np.array([3.0, 5.0, 11.0]) ** 2)) == [7, 5, 3]
    with pytest.raises(ValueError):
        ff.force_constant(i, j, np.array([3.0, 5.0, 13.0]) ** 2)
    with pytest.raises(IndexError):
        sc.TabulatedForceField(atoms, [1, 2], 1, 1, edges)
    with pytest.raises(ValueError):
        sc.TabulatedForceField(atoms, 1, np.arange(400.0).reshape(20, 20), 1, 5.0)   # not symmetric
    with pytest.raises(TypeError):
        sc.TabulatedForceField(np.zeros((6, 3)), 1, 1, 1, 5.0)
    bad = atoms.copy()
    bad.atom_name[0] = "CB"
    with pytest.raises(sc.atoms.BadStructureError):
        sc.TabulatedForceField(bad, 1, 1, 1, 5.0)


def test_model_validation_without_gpu():
    import springcraft_amd as sc

    coord = np.random.RandomState(0).rand(10, 3)
    ff = sc.InvariantForceField(5.0)
    with pytest.raises(TypeError):
        sc.ANM(coord, ff, masses=True)
    atoms = sc.AtomArray(10)
    atoms.coord = coord
    with pytest.raises(IndexError):
        sc.ANM(atoms, ff, masses=np.ones(9))
    with pytest.raises(ValueError):
        sc.GNM(atoms, ff, masses=np.zeros(10))
    anm = sc.ANM(atoms, ff, masses=np.full(10, 4.0))
    assert np.allclose(anm._inv_sqrt_mass, 0.5) and anm.masses.shape == (10,)
    h = np.eye(30)
    anm.hessian = h
    assert anm.hessian is h                                   # not a copy (anm.py:53)
    c = 2 * np.eye(30)
    anm.covariance = c                                         # invalidates the Hessian (anm.py:138-148)
    assert anm.covariance is c and anm._matrix is None


def test_shard_bounds():
    from springcraft_amd.batch import shard_bounds

    for n_items, world in [(256, 8), (10, 3), (3, 8), (0, 4)]:
        spans = [shard_bounds(n_items, world, r) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n_items
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1


def test_pdb_adaptor_and_residue_masses():
    """F4 input adaptor: C-alpha reader (filter of tests/test_anm.py:17-18) + masses for ``masses=True``."""
    import springcraft_amd as sc
    from tests.util import ref_data, structures

    ca = sc.read_pdb_ca(ref_data("1l2y.pdb"))
    s = structures()
    assert ca.array_length() == 20
    assert np.array_equal(ca.coord, s["1l2y_coord"]) and ca.coord.dtype == np.float32
    assert list(ca.res_name) == list(s["1l2y_res_name"])
    assert list(ca.res_id) == list(s["1l2y_res_id"])
    anm = sc.ANM(ca, sc.InvariantForceField(13.0), masses=True)
    # masses=True uses the free amino-acid masses (what biotite's info.mass(res_name, is_residue=True) reports)
    assert anm.masses.shape == (20,)
    assert anm.masses[0] == pytest.approx(132.118) and anm.masses[9] == pytest.approx(75.067)   # ASN, GLY


def test_host_logic_under_sanitizers(tmp_path):
    """
    SURVEY section 5: sanitizers on the CPU build only.  The HIP-free host logic of the C ABI (contact-patch override
    table, force-field descriptor checks: csrc/host_logic.h, included by the api_*.hip units) compiled with g++ under ASan + UBSan
    and driven through its edge cases (tests/host_sanitize/test_host_logic.cpp).
    """
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_host_logic")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_host_logic.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host logic ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


EIGH_ENV = ("SPRINGCRAFT_NB", "SPRINGCRAFT_TWO_STAGE", "SPRINGCRAFT_NO_AUX", "SPRINGCRAFT_AUX_SINGLE", "SPRINGCRAFT_RESIDENT",
            "SPRINGCRAFT_RESIDENT_WGS", "SPRINGCRAFT_RESIDENT_MAX", "SPRINGCRAFT_RESIDENT_NO_CHAIN", "SPRINGCRAFT_RESIDENT_DELAY")


def test_eigh_policy_under_sanitizers(tmp_path):
    """
    The eigensolver's top-level policy (csrc/eigh_policy.h: panel width, one-stage or two-stage, what forks onto the second
    stream) compiled with g++ under ASan + UBSan and checked against literals (tests/host_sanitize/test_eigh_policy.cpp).
    """
    import os
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_eigh_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_eigh_policy.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in EIGH_ENV}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "eigh policy ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_stedc_plan_under_sanitizers(tmp_path):
    """
    The plan of the tridiagonal divide & conquer (csrc/stedc_plan.h: the merge tree, the launch shapes and LDS bytes of a
    level's kernels, buffer parity, the layout of the auxiliary buffer) compiled with g++ under ASan + UBSan and checked
    against literals (tests/host_sanitize/test_stedc_plan.cpp).
    """
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_stedc_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_stedc_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stedc plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_sy2sb_plan_under_sanitizers(tmp_path):
    """
    The plan of the band reduction (csrc/sy2sb_plan.h: panel geometry, the GEMM records of a solve and their places, the
    LDS layouts of the stage-1 kernels, k_panel_coop's carve of the auxiliary buffer, the parts of a split batch) compiled
    with g++ under ASan + UBSan and checked against literals (tests/host_sanitize/test_sy2sb_plan.cpp).
    """
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_sy2sb_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_sy2sb_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sy2sb plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# sc_eigh_workspace_bytes(n, batch, want_vectors = 0 / 1) of the revision before the drivers shared one plan (taken from that
# revision's library on the host: the function needs neither a context nor a device), default environment
EIGH_WORKSPACE_BYTES = {
    (1, 1): (9472, 2914048),
    (63, 1): (139264, 4261376),
    (300, 1): (662528, 13465088),
    (300, 4): (2646016, 53854720),
    (520, 64): (1159998464, 2611284992),
    (2000, 16): (1762477568, 3751801600),
    (6000, 4): (3100750336, 6128908800),
    (8000, 1): (1376765440, 2642096896),
    # (above both LDS caps of the D&C; of the revision before its plan header)
    (7001, 2): (2075222784, 4066082048),
    (9801, 3): (5750026496, 11246490880),
}


def test_eigh_workspace_totals_unchanged():
    """One plan for every kind of solve carves the full-spectrum workspace to the byte as the two plans before it did."""
    import os

    from springcraft_amd import _hip

    L = _hip.lib()
    for (n, batch), want in EIGH_WORKSPACE_BYTES.items():
        got = (L.sc_eigh_workspace_bytes(n, batch, 0), L.sc_eigh_workspace_bytes(n, batch, 1))
        assert got == want, (n, batch, got, want, "set in the environment:", [k for k in EIGH_ENV if k in os.environ])


def test_hip_sources_compile_without_warnings(tmp_path):
    """
    Every HIP source compiles for gfx950 with -Wall and no warning (a missing return slipped through once in round 2 and
    only showed as a warning).  Objects go to a scratch directory; the in-tree library is not touched.
    """
    import shutil
    import subprocess

    from springcraft_amd.csrc import build as b

    if shutil.which(b.HIPCC) is None:
        pytest.skip("hipcc not available")
    out = []
    for src in b.sources():
        cmd = [b.HIPCC, "-c", join(b.HERE, src), "-o", str(tmp_path / (src + ".o"))] + b.COMMON + b.PER_FILE.get(src, [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{src}:\n{r.stderr[-3000:]}"
        if "warning" in r.stderr:
            out.append(f"{src}:\n{r.stderr}")
    assert not out, "\n".join(out)[-4000:]


def test_host_array_without_a_device():
    """Result arrays: small ones are ordinary NumPy arrays; large ones fall back to ordinary memory when the runtime cannot
    page-lock (no GPU here) -- either way a writable C-contiguous float64 ndarray of the requested shape."""
    from springcraft_amd import _hip

    for shape in ((7,), (10, 10), (1100, 1100)):
        a = _hip.host_array(shape)
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.float64
        assert a.flags.c_contiguous and a.flags.writeable
        a[...] = 1.0
        assert float(a.sum()) == float(np.prod(shape))
