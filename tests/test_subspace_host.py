"""
CPU-only checks of the pairwise comparison of mode subspaces (``_BatchSolver.rmsip`` / ``covariance_overlap`` /
``mode_overlap_matrix``, ``nma.rmsip`` / ``covariance_overlap`` / ``mode_overlap_matrix``): the public names, header against
symbol table against binding for the three C entries, the errors that are raised on the host before the library or a device
is touched, the NumPy specification of tests/subspace.py against an independent reference and against the identities it
must satisfy, and the specification in extended precision against the derived bound on the inputs the GPU tests use.
"""
import inspect
import re
from os.path import dirname, join

import numpy as np
import pytest

from oracle import enm_oracle as orc
from tests.subspace import (CUTOFF, EPS, cov_weights, ensemble, np_cov_overlap, np_gram, np_rmsip, np_S, pinv_rows,
                            ref_cov_overlap, s_bound)

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_subspace": 10, "sc_dev_subspace_f64": 19, "sc_dev_subspace_gram_f64": 15}


def no_device(*a, **k):
    raise AssertionError("the check must not reach the native library")


@pytest.fixture
def host_only(monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)


def _fake_solver(dim, ragged=False, n_atoms=5, batch=3, device=0):
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
        s._layout = B._UniformLayout(batch, n_atoms, dim)
        s.batch, s.n_atoms, m = batch, n_atoms, dim * n_atoms
    s.torch, s.dim, s.device = torch, dim, torch.device("cuda", device)
    s.window, s.subset, s.counts, s._first_row, s._common_modes = None, None, None, 0, m
    s.w = torch.zeros((s.batch, m), dtype=torch.float64)
    s.v = torch.zeros((s.batch, m, m), dtype=torch.float64)
    s._L, s.ctx, s._plan = None, None, None
    return s


def test_public_names_and_signatures():
    import springcraft_amd as sc
    from springcraft_amd import batch, nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    base = batch._BatchSolver
    for cls in (DeviceBatchSolver, RaggedBatchSolver, sc.RTB):
        for name in ("rmsip", "covariance_overlap", "mode_overlap_matrix"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(base, name)

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(base.rmsip) == [("self", E), ("n_modes", 10), ("mode_subset", None), ("other", None)]
    assert params(base.covariance_overlap) == [("self", E), ("mode_subset", None), ("other", None)]
    assert params(base.mode_overlap_matrix) == [("self", E), ("pairs", E), ("mode_subset", E), ("other", None)]
    assert params(nma.rmsip) == [("enm_a", E), ("enm_b", E), ("n_modes", 10), ("mode_subset", None)]
    assert params(nma.covariance_overlap) == [("enm_a", E), ("enm_b", E), ("mode_subset", None)]
    assert params(nma.mode_overlap_matrix) == [("enm_a", E), ("enm_b", E), ("mode_subset_a", E), ("mode_subset_b", None)]
    for name in ("rmsip", "covariance_overlap", "mode_overlap_matrix"):
        assert name in nma.__all__
        for cls in (sc.ANM, sc.GNM):
            assert list(inspect.signature(getattr(cls, name)).parameters)[:2] == ["self", "other"]
    assert "atom_scale" not in inspect.signature(base.rmsip).parameters and "out of scope" in base.rmsip.__doc__


def test_header_symbol_table_and_binding_name_the_three_entries():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "subspace" in n}
    assert declared == set(ENTRIES)
    assert {n for n in _hip.EXPORTED_SYMBOLS if "subspace" in n} == set(ENTRIES)
    taken = ("prs", "overlap", "msf", "dcc", "aniso", "distfluct", "response", "combine")
    assert not [n for n in ENTRIES for word in taken if word in n]
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name
    assert callable(_hip.Modes.subspace)


def test_batch_errors_are_raised_on_the_host(host_only):
    rag = _fake_solver(3, ragged=True)
    for call in (rag.rmsip, rag.covariance_overlap, lambda: rag.mode_overlap_matrix([(0, 1)], [7])):
        with pytest.raises(ValueError, match="members of different size have no common coordinates"):
            call()
    s = _fake_solver(3)
    with pytest.raises(ValueError, match="members of different size have no common coordinates"):
        s.rmsip(other=rag)
    for other, why in ((_fake_solver(3, n_atoms=6), "6 atoms"), (_fake_solver(1, n_atoms=5), "dim = 1"),
                       (_fake_solver(3, device=1), "cuda:1"), (np.zeros((3, 15, 15)), "uniform batch solver")):
        for call in (lambda: s.rmsip(other=other), lambda: s.covariance_overlap(other=other),
                     lambda: s.mode_overlap_matrix([(0, 0)], [7], other=other)):
            with pytest.raises(ValueError, match=why):
                call()
    streamed = _fake_solver(3)
    streamed._stream = 1234
    with pytest.raises(ValueError, match="another stream"):
        s.rmsip(other=streamed)
    novec = _fake_solver(3)
    novec.v = None
    for call in (novec.rmsip, novec.covariance_overlap, lambda: novec.mode_overlap_matrix([(0, 1)], [7]),
                 lambda: s.rmsip(other=novec)):
        with pytest.raises(ValueError, match="want_vectors=True"):
            call()
    small = _fake_solver(3, batch=2)
    for pairs in ([(0, 3)], [(3, 0)], [(0, 1), (-1, 0)]):
        with pytest.raises(ValueError, match="pairs must name members"):
            s.mode_overlap_matrix(pairs, [7, 8])
    with pytest.raises(ValueError, match=r"0 <= b < 2"):
        s.mode_overlap_matrix([(2, 2)], [7, 8], other=small)
    for pairs in ([0, 1], [(0.0, 1.0)], [(0, 1, 2)]):
        with pytest.raises(ValueError, match="pairs must be"):
            s.mode_overlap_matrix(pairs, [7])
    with pytest.raises(ValueError, match="explicit mode_subset"):
        s.mode_overlap_matrix([(0, 1)], None)
    for call in (lambda sub: s.rmsip(mode_subset=sub), lambda sub: s.covariance_overlap(sub),
                 lambda sub: s.mode_overlap_matrix([(0, 1)], sub)):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            call([5, 7])
        with pytest.raises(ValueError, match="mode 15 was not solved"):
            call([7, 15])
    with pytest.raises(ValueError, match="n_modes must not be negative"):
        s.rmsip(n_modes=-1)
    windowed = _fake_solver(3)
    windowed.window = (0.1, 2.0)
    for call in (lambda: windowed.rmsip(mode_subset=[7]), lambda: windowed.covariance_overlap([7]),
                 lambda: windowed.mode_overlap_matrix([(0, 1)], [7])):
        with pytest.raises(ValueError, match="subset_by_value"):
            call()


def test_one_model_errors_are_raised_on_the_host(host_only):
    import springcraft_amd as sc
    from springcraft_amd import nma

    coord = np.random.RandomState(0).rand(10, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    anm, gnm, anm9 = sc.ANM(coord, ff), sc.GNM(coord, ff), sc.ANM(coord[:9], ff)
    for f in (lambda a, b: nma.rmsip(a, b), lambda a, b: nma.covariance_overlap(a, b),
              lambda a, b: nma.mode_overlap_matrix(a, b, [7]), lambda a, b: a.rmsip(b), lambda a, b: a.covariance_overlap(b),
              lambda a, b: a.mode_overlap_matrix(b, [7])):
        with pytest.raises(ValueError, match="Cannot compare the modes of a ANM with those of a GNM"):
            f(anm, gnm)
        with pytest.raises(ValueError, match="10 and 9 atoms"):
            f(anm, anm9)
    with pytest.raises(ValueError, match="Instance of GNM/ANM class expected"):
        nma.rmsip(anm, np.eye(30))
    for f in (lambda sub: nma.rmsip(anm, anm, mode_subset=sub), lambda sub: nma.covariance_overlap(anm, anm, sub),
              lambda sub: nma.mode_overlap_matrix(anm, anm, sub), lambda sub: nma.mode_overlap_matrix(anm, anm, [7], sub)):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            f([5, 7])
    with pytest.raises(ValueError, match="n_modes must not be negative"):
        nma.rmsip(anm, anm, n_modes=-2)


_CASES = {}


def lapack_case(n_atoms, batch=3, dim=3):
    """LAPACK eigenpairs (rows = modes) of the oracle's matrices of the ensemble the GPU tests solve: once per shape."""
    key = (n_atoms, batch, dim)
    if key not in _CASES:
        out = []
        for c in ensemble(n_atoms, batch):
            mat = orc.compute_hessian(c, orc.invariant_ff(CUTOFF))[0] if dim == 3 else \
                orc.compute_kirchhoff(c, orc.invariant_ff(10.0))[0]
            w, vec = np.linalg.eigh(mat)
            out.append((w, np.ascontiguousarray(vec.T)))
        _CASES[key] = out
    return _CASES[key]


def test_the_covariance_overlap_is_the_dense_formula():
    (wa, va), (wb, vb), _ = lapack_case(24)
    # (distinct modes: S stands for tr(sqrt(A) sqrt(B)) only while each set is orthonormal)
    for rows in (np.arange(6, 72), np.arange(6, 16), [30, 6, 9, 12]):
        got, ref = np_cov_overlap(wa, va, wb, vb, rows, rows), ref_cov_overlap(wa, va, wb, vb, rows, rows)
        # the root of a difference of traces that cancels: d^2 = (1 - omega)^2 (T_a + T_b) carries about 100 eps (T_a + T_b)
        assert 0.0 < got < 1.0 and abs(got - ref) <= 100 * EPS / max(1 - ref, 1e-3), (rows, got, ref)
    ra, rb = pinv_rows(wa), pinv_rows(wb)
    assert np.array_equal(ra, np.arange(6, 72))
    assert abs(np_cov_overlap(wa, va, wa, va, ra, ra) - 1) <= 1e-6
    assert abs(np_cov_overlap(wa, va, wb, vb, ra, rb) - np_cov_overlap(wb, vb, wa, va, rb, ra)) <= 1e-13


def test_rmsip_identities():
    (wa, va), (wb, vb), _ = lapack_case(24)
    rows = np.arange(6, 16)
    assert abs(np_rmsip(va, va, rows, rows) - 1) <= 1e-13
    # a rotation of the set within its span spans the same subspace
    q, _ = np.linalg.qr(np.random.RandomState(2).randn(10, 10))
    rot = va.copy()
    rot[rows] = q @ va[rows]
    assert abs(np_rmsip(va, rot, rows, rows) - 1) <= 1e-13
    # two different sets: strictly between 0 and 1, symmetric, and Amadei's formula
    r = np_rmsip(va, vb, rows, rows)
    assert 0.3 < r < 0.999 and abs(r - np_rmsip(vb, va, rows, rows)) <= 1e-14
    assert abs(r - np.sqrt((np_gram(va, vb, rows, rows) ** 2).sum() / 10)) <= 1e-15
    # unequal counts stay defined; a mode listed twice counts twice; nothing listed is 0 / 0
    assert 0 < np_rmsip(va, vb, rows, rows[:7]) < 1
    assert abs(np_S(va, vb, [7, 7], [8], [1, 1], [1]) - 2 * np_S(va, vb, [7], [8], [1], [1])) <= 1e-16
    assert np.isnan(np_rmsip(va, vb, [], []))
    # all m modes of two different complete orthonormal sets: S = m, RMSIP = 1
    full = np.arange(72)
    assert abs(np_S(va, vb, full, full, np.ones(72), np.ones(72)) - 72) <= s_bound(72, 72, 72)
    assert abs(np_rmsip(va, vb, full, full) - 1) <= 1e-13


@pytest.mark.parametrize("n_atoms,dim", [(7, 3), (24, 3), (67, 3), (33, 1)])
def test_the_model_in_extended_precision_stays_inside_the_bound(n_atoms, dim):
    """float64 against longdouble on the GPU tests' ensembles and selections: the gate is one the model itself passes."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("this platform's long double is a double")
    cases = lapack_case(n_atoms, 3, dim)
    m, ntriv = dim * n_atoms, 6 if dim == 3 else 1
    lists = [np.arange(ntriv, ntriv + k) for k in (1, 3, 16, 17, 65) if ntriv + k <= m] + [np.arange(ntriv, m)]
    worst = 0.0
    for (wa, va), (wb, vb) in ((cases[0], cases[1]), (cases[2], cases[0]), (cases[1], cases[1])):
        for rows in lists:
            for weights in ("unit", "covariance"):
                if weights == "unit":
                    pa = pb = np.ones(len(rows))
                    pal = pbl = np.ones(len(rows), dtype=np.longdouble)
                else:
                    pa, pb = cov_weights(wa, rows), cov_weights(wb, rows)
                    pal, pbl = cov_weights(wa, rows, np.longdouble), cov_weights(wb, rows, np.longdouble)
                model = np_S(va, vb, rows, rows, pa, pb)
                exact = np_S(va, vb, rows, rows, pal, pbl, dtype=np.longdouble)
                ratio = float(abs(model - exact) / s_bound(m, pa.sum(), pb.sum()))
                worst = max(worst, ratio)
                # the model's own error is half of what the bound allows between two computed values
                assert ratio <= 0.5, (n_atoms, dim, len(rows), weights, ratio)
    print(f"N = {n_atoms} dim {dim}: float64 model against long double, max |difference| / bound = {worst:.3e}")
