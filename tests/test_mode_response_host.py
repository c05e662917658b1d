"""
CPU-only checks of the linear response and the mode synthesis (``nma.linear_response``, ``nma.mode_displacement``,
``nma.sample_displacements`` and the batch solvers' ``linear_response`` / ``mode_displacement``): the public names, the
errors that are raised on the host before the library or a device is touched, the layout of the packed (q, sum n, dim)
result of a ragged batch, the coefficients ``sample_displacements`` draws against their NumPy expression, and header
against binding for the six C entries, the way tests/test_abi_and_host.py checks the whole ABI.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_modes_response", "sc_dev_mode_response_f64", "sc_batch_plan_mode_response_f64",
           "sc_modes_combine", "sc_dev_mode_combine_f64", "sc_batch_plan_mode_combine_f64"}


def no_device(*a, **k):
    raise AssertionError("the check must not reach the native library")


@pytest.fixture
def host_only(monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_hip, "context", no_device)


def models(n=10):
    import springcraft_amd as sc

    coord = np.random.RandomState(0).rand(n, 3) * 8.0
    ff = sc.InvariantForceField(7.0)
    return sc.ANM(coord, ff), sc.GNM(coord, ff)


def test_public_names():
    import springcraft_amd as sc
    from springcraft_amd import nma
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    for name in ("linear_response", "mode_displacement", "sample_displacements"):
        assert name in nma.__all__ and callable(getattr(sc.nma, name))
    assert callable(sc.ANM.linear_response) and callable(sc.ANM.mode_displacement) and callable(sc.GNM.mode_displacement)
    assert not hasattr(sc.GNM, "linear_response")
    for cls in (DeviceBatchSolver, RaggedBatchSolver):
        assert callable(cls.linear_response) and callable(cls.mode_displacement)
    for fn in (nma.mode_displacement, nma.sample_displacements, DeviceBatchSolver.mode_displacement):
        assert "no reference counterpart" in fn.__doc__.lower()
    assert "host arithmetic" not in nma.__doc__.split("linear_response")[1].split("normal_mode")[0]


def test_linear_response_errors_are_raised_on_the_host(host_only):
    from springcraft_amd import nma

    n = 10
    anm, gnm = models(n)
    for not_an_anm in (gnm, np.eye(30), None):
        with pytest.raises(ValueError, match="Instance of ANM class expected"):
            nma.linear_response(not_an_anm, np.zeros((n, 3)))
    # the reference's errors, with their messages (nma.py:456-471)
    with pytest.raises(ValueError, match=r"Expected force with shape \(10, 3\), got \(11, 3\)"):
        nma.linear_response(anm, np.zeros((n + 1, 3)))
    with pytest.raises(ValueError, match=r"Expected force with shape \(10, 3\), got \(10, 2\)"):
        anm.linear_response(np.zeros((n, 2)))
    with pytest.raises(ValueError, match="Expected force with length 30, got 29"):
        nma.linear_response(anm, np.zeros(29))
    for bad in (np.zeros((2, 2, n, 3)), 1.0):
        with pytest.raises(ValueError, match="Expected 1D or 2D array"):
            nma.linear_response(anm, bad)
    # q forces at once
    for bad in (np.zeros((2, n + 1, 3)), np.zeros((2, n, 2)), np.zeros((n, 3, 1))):
        with pytest.raises(ValueError, match=r"Expected forces with shape \('q', 10, 3\)"):
            nma.linear_response(anm, bad)
    for subset in ([5, 7], np.arange(0, 12), [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.linear_response(anm, np.ones((n, 3)), mode_subset=subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            anm.linear_response(np.ones((2, n, 3)), subset)


def test_a_covariance_on_the_model_is_applied_as_it_is(host_only):
    """The rule of prs: an assigned covariance is that very matrix, also for q forces at once; no device is asked."""
    n = 10
    anm, _ = models(n)
    rs = np.random.RandomState(1)
    a = rs.randn(3 * n, 3 * n)
    anm.covariance = a
    f = rs.randn(4, n, 3)
    assert np.array_equal(anm.linear_response(f[2]), (a @ f[2].ravel()).reshape(n, 3))
    assert np.array_equal(anm.linear_response(f[2].ravel()), (a @ f[2].ravel()).reshape(n, 3))
    got = anm.linear_response(f)
    assert got.shape == (4, n, 3)
    assert np.allclose(got, np.stack([(a @ x.ravel()).reshape(n, 3) for x in f]), rtol=1e-13, atol=1e-13)
    assert anm.linear_response(np.zeros((0, n, 3))).shape == (0, n, 3)


def test_mode_displacement_errors_are_raised_on_the_host(host_only):
    from springcraft_amd import nma

    n = 10
    anm, gnm = models(n)
    with pytest.raises(ValueError, match="Instance of GNM/ANM class expected"):
        nma.mode_displacement(np.eye(30), np.zeros(24))
    with pytest.raises(ValueError, match="Instance of GNM/ANM class expected"):
        nma.sample_displacements(None, 3)
    for bad in (np.zeros(30), np.zeros(23), np.zeros((2, 25)), np.zeros((2, 2, 24)), 1.0):
        with pytest.raises(ValueError, match=r"Expected coefficients of shape \(24,\) or \(q, 24\)"):
            nma.mode_displacement(anm, bad)
    with pytest.raises(ValueError, match=r"Expected coefficients of shape \(9,\) or \(q, 9\)"):
        gnm.mode_displacement(np.zeros(10))
    with pytest.raises(ValueError, match=r"Expected coefficients of shape \(3,\) or \(q, 3\)"):
        anm.mode_displacement(np.zeros((2, 4)), mode_subset=[7, 9, 7])
    for subset in ([5, 7], [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.mode_displacement(anm, np.zeros(len(subset)), subset)
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            nma.sample_displacements(anm, 2, mode_subset=subset)
    with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
        gnm.mode_displacement(np.zeros(2), mode_subset=[0, 3])
    with pytest.raises(ValueError, match="n_samples"):
        nma.sample_displacements(anm, -1)


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


def test_batch_errors_are_raised_on_the_host(host_only):
    import torch

    s = _fake_solver(3)
    good = torch.zeros((3, 5, 3), dtype=torch.float64)
    # (no test machine without a device can make a CUDA tensor: every tensor here fails the first check, as a CPU tensor)
    for bad in (good, good.numpy(), good.float(), torch.zeros((3, 3, 5), dtype=torch.float64).transpose(1, 2)):
        with pytest.raises(ValueError, match="force must be a contiguous CUDA float64 tensor of shape .*batch, q, N, 3"):
            s.linear_response(bad)
    for bad in (torch.zeros((3, 15), dtype=torch.float64), np.zeros((3, 15)),
                torch.zeros((3, 15, 2), dtype=torch.float64).transpose(1, 2)):
        with pytest.raises(ValueError, match="coefficients must be a contiguous CUDA float64 tensor of shape .*batch, q, nvec"):
            s.mode_displacement(bad)
    gnm = _fake_solver(1)
    with pytest.raises(ValueError, match="linear_response needs an ANM solver"):
        gnm.linear_response(torch.zeros((3, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="coefficients must be a contiguous CUDA float64"):
        gnm.mode_displacement(torch.zeros((3, 5), dtype=torch.float64))      # dim 1 is allowed: the tensor check is next
    rag = _fake_solver(3, ragged=True)
    with pytest.raises(ValueError, match=r"force must be .*\(S, 3\) or \(q, S, 3\) with S = sum\(sizes\) = 10"):
        rag.linear_response(torch.zeros((10, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="linear_response needs an ANM solver"):
        _fake_solver(1, ragged=True).linear_response(torch.zeros((10,), dtype=torch.float64))
    novec = _fake_solver(3)
    novec.v = None
    with pytest.raises(ValueError, match="want_vectors=True"):
        novec.linear_response(good)
    with pytest.raises(ValueError, match="want_vectors=True"):
        novec.mode_displacement(torch.zeros((3, 15), dtype=torch.float64))


def test_force_shapes_use_the_displacement_rule_and_say_force():
    from springcraft_amd.batch import _RaggedLayout, _UniformLayout

    uni = _UniformLayout(3, 5, 3)
    assert uni.displacement_q((3, 5, 3), "force") == (1, True) and uni.displacement_q((3, 4, 5, 3), "force") == (4, False)
    with pytest.raises(ValueError, match=r"Expected a force of shape \(batch, N, 3\) or \(batch, q, N, 3\)"):
        uni.displacement_q((3, 5), "force")
    with pytest.raises(ValueError, match="Expected a displacement of shape"):
        uni.displacement_q((3, 5))
    rag = _RaggedLayout((4, 6), 1, [4, 6])
    with pytest.raises(ValueError, match=r"Expected a force of shape \(S,\) or \(q, S\) with S = sum\(sizes\) = 10"):
        rag.displacement_q((10, 3), "force")


@pytest.mark.parametrize("dim", [3, 1])
def test_layout_of_q_vectors_per_structure(dim):
    import torch

    from springcraft_amd.batch import _RaggedLayout, _UniformLayout

    tail = (3,) if dim == 3 else ()
    sizes = (4, 6, 5)
    total = sum(sizes)
    lay = _RaggedLayout(sizes, dim, [dim * n for n in sizes])
    assert lay.vectors_shape(1) == (1, total) + tail and lay.vectors_shape(4) == (4, total) + tail
    assert lay.vectors_shape(0) == (0, total) + tail
    buf = torch.arange(4 * total * dim, dtype=torch.float64).reshape((4, total) + tail)
    many, one = lay.vectors_out(buf), lay.vectors_out(buf[:1], single=True)
    assert len(many) == len(one) == len(sizes)
    off = 0
    for b, n in enumerate(sizes):
        assert tuple(many[b].shape) == (4, n) + tail and tuple(one[b].shape) == (n,) + tail
        assert torch.equal(many[b], buf[:, off: off + n]) and torch.equal(one[b], buf[0, off: off + n])
        # views into the one packed buffer, at the structure's atom offset: force j at stride dim * sum n
        assert many[b].untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        assert many[b].storage_offset() == dim * off and one[b].storage_offset() == dim * off
        assert many[b].stride(0) == dim * total
        off += n
    many[1][2] = -1.0
    assert bool((buf[2, 4:10] == -1.0).all()) and int((buf == -1.0).sum()) == 6 * dim
    assert [tuple(t.shape) for t in lay.vectors_out(buf[:0])] == [(0, n) + tail for n in sizes]

    uni = _UniformLayout(3, 5, dim)
    assert uni.vectors_shape(4) == (3, 4, 5) + tail
    ubuf = torch.zeros(uni.vectors_shape(4), dtype=torch.float64)
    assert uni.vectors_out(ubuf) is ubuf
    single = uni.vectors_out(ubuf[:, :1], single=True)
    assert tuple(single.shape) == (3, 5) + tail and single.untyped_storage().data_ptr() == ubuf.untyped_storage().data_ptr()


@pytest.mark.parametrize("kind", ["anm", "gnm"])
def test_sample_displacements_coefficients(monkeypatch, kind):
    """xi sqrt(kT / lambda) with xi from numpy.random.default_rng(rng), handed to mode_displacement with the selection."""
    from springcraft_amd import nma

    n = 10
    anm, gnm = models(n)
    enm, ntriv, order = (anm, 6, 30) if kind == "anm" else (gnm, 1, 10)
    lam = np.linspace(0.5, 4.0, order)
    lam[:ntriv] = 0.0
    seen = {}

    class Stub:
        def values(self):
            return lam.copy()

    def fake_mode_displacement(model, coefficients, mode_subset=None):
        seen["args"] = (model, np.array(coefficients), None if mode_subset is None else np.array(mode_subset))
        return "the displacement"

    monkeypatch.setattr(type(enm), "_modes_device", lambda self: Stub())
    monkeypatch.setattr(nma, "mode_displacement", fake_mode_displacement)
    for subset, tem, factors in ((None, None, nma.K_B), ([ntriv + 2, ntriv, order - 1], 300.0, nma.K_B), ([ntriv + 1], 2.0, 0.5)):
        idx = np.arange(ntriv, order) if subset is None else np.array(subset)
        kt = 1.0 if tem is None else tem * factors
        out = nma.sample_displacements(enm, 7, mode_subset=subset, tem=tem, tem_factors=factors, rng=42)
        assert out == "the displacement"
        model, coef, passed = seen["args"]
        assert model is enm and np.array_equal(passed, idx)
        xi = np.random.default_rng(42).standard_normal((7, len(idx)))
        assert coef.shape == (7, len(idx)) and np.array_equal(coef, xi * np.sqrt(kt / lam[idx]))
    # a Generator is taken as it is, and advances
    gen = np.random.default_rng(3)
    nma.sample_displacements(enm, 2, rng=gen)
    first = seen["args"][1]
    nma.sample_displacements(enm, 2, rng=gen)
    assert not np.array_equal(first, seen["args"][1])
    nma.sample_displacements(enm, 0, rng=1)
    assert seen["args"][1].shape == (0, order - ntriv)


def test_header_declares_the_six_entries_and_the_binding_binds_them():
    from springcraft_amd import _hip

    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = {n for n in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header) if "response" in n or "combine" in n}
    assert declared == ENTRIES
    assert {n for n in _hip.EXPORTED_SYMBOLS if "response" in n or "combine" in n} == ENTRIES
    proto = {
        "sc_dev_mode_response_f64":
            r"int sc_dev_mode_response_f64\(sc_ctx\* ctx, const double\* d_w, const double\* d_v, int64_t m, int64_t nvec, "
            r"int64_t batch,\s+int dim, const sc_mode_selection\* sel, const int64_t\* d_counts, const double\* d_force,\s+"
            r"int64_t q, const double\* d_atom_scale, double\* d_out\);",
        "sc_dev_mode_combine_f64":
            r"int sc_dev_mode_combine_f64\(sc_ctx\* ctx, const double\* d_v, int64_t m, int64_t nvec, int64_t batch, "
            r"int dim,\s+const double\* d_coef, int64_t q, const int64_t\* d_counts, const double\* d_atom_scale,\s+"
            r"double\* d_out\);",
        "sc_modes_combine":
            r"int sc_modes_combine\(sc_modes\* modes, const int64_t\* mode_idx, int64_t k, const double\* coef, int64_t q, "
            r"double\* out\);",
    }
    for name, pat in proto.items():
        assert re.search(pat, header), name
    L = _hip.lib()
    nargs = {"sc_dev_mode_response_f64": 13, "sc_batch_plan_mode_response_f64": 10, "sc_modes_response": 8,
             "sc_dev_mode_combine_f64": 11, "sc_batch_plan_mode_combine_f64": 9, "sc_modes_combine": 6}
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs[name], name
    assert callable(_hip.Modes.response) and callable(_hip.Modes.combine)


def test_workspace_codes_5_and_6():
    """Response: weights + the coefficients of four forces + partial sums; combine: the partial sums.  From (m, rows, budget)."""
    from springcraft_amd import _hip

    ws = _hip.lib().sc_dev_modes_workspace_bytes
    m, nsel = 513, 507                                      # chunks of msf_chunk(507) = 11 rows: 47 of them
    nchunk = -(-nsel // max(4, -(-nsel // 48)))
    assert nchunk == 47

    def up(x):
        return -(-x // 256) * 256

    for batch in (1, 3):
        part = up(batch * nchunk * 4 * m * 8)
        assert ws(m, m, batch, 3, nsel, 6, 0) == part + 1024
        assert ws(m, m, batch, 3, nsel, 5, 0) == up(batch * nsel * 8) + up(batch * 4 * nsel * 8) + part + 1024
    # a budget of one structure's partial sums: the slab is one structure, whatever the batch
    one = nchunk * 4 * m * 8
    assert ws(m, m, 7, 3, nsel, 6, one) == up(one) + 1024
    assert ws(m, m, 7, 3, nsel, 6, 0) == up(7 * one) + 1024
    assert ws(m, m, 3, 1, nsel, 6, 0) == ws(m, m, 3, 3, nsel, 6, 0) > 0      # GNM too
    # the other codes answer as before
    assert ws(m, m, 3, 3, nsel, 3, 0) == 0 and ws(m, m, 3, 3, nsel, 0, 0) > 0


def test_the_field_entry_table_names_the_four_batch_entries_once():
    """What tests/test_batch_layout_host.py asserts of _CONSUMER_ENTRIES, for the table of the displacement-field consumers."""
    from springcraft_amd import _hip, batch

    names = [n for row in batch._FIELD_ENTRIES.values() for n in (row[0], row[2])]
    assert len(names) == len(set(names)) == 4
    assert set(names) == {s for s in _hip.EXPORTED_SYMBOLS if s.startswith(("sc_dev_mode_", "sc_batch_plan_mode_"))}
    assert not set(batch._FIELD_ENTRIES) & set(batch._CONSUMER_ENTRIES)
    source = open(batch.__file__).read()
    for n in names:
        assert source.count(n) == 1, n
    for uniform, uniform_prefix, plan, plan_prefix in batch._FIELD_ENTRIES.values():
        assert uniform.startswith("sc_dev_mode_") and uniform_prefix[0] == "ctx"
        assert plan == uniform.replace("sc_dev_mode_", "sc_batch_plan_mode_") and plan_prefix[0] == "plan"
    for cls in (batch.DeviceBatchSolver, batch.RaggedBatchSolver):
        for name in ("linear_response", "mode_displacement"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(batch._BatchSolver, name)
