"""
GPU tests of the mode overlaps and collectivities (``k_modes_overlap`` of csrc/mode_overlap.hip) through the three layers:
``nma.overlap`` / ``nma.collectivity`` (one model, ``sc_modes_overlap``), ``DeviceBatchSolver``
(``sc_dev_modes_overlap_f64``) and ``RaggedBatchSolver`` (``sc_batch_plan_modes_overlap_f64``).

Ground truth is NumPy on the solver's own eigenvectors,

    O[j, r] = <v_r, d_j> / (|v_r| |d_j|) = (V @ d_j) / (norms of the rows of V * |d_j|)
    kappa[r] = exp(-sum_a p_a ln p_a) / N,   p_a = s_a / sum s,   s_a = sum_c V[r, dim a + c]^2      (two passes)

under ``np.allclose`` with its defaults, the gate of the other consumer tests.  Placement checks are bit for bit.  Shapes
are the smallest that reach each branch: N = 20 (a row shorter than a wavefront), 37 (m = 111 odd: 8-byte loads and an
atom without a partner), 171 (m = 513 odd, more than one trip of the lanes), 257 (m = 771).
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests.test_batch_consumers_gpu import make_coords, solved, window_case
from tests.util import ref_data, synthetic_coord

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def np_overlap(v, d):
    """(q, k): rows of v (k, m) against the vectors d (q, m)."""
    d = d.reshape(len(d), -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d @ v.T) / (np.linalg.norm(d, axis=1)[:, None] * np.linalg.norm(v, axis=1)[None, :])


def np_collectivity(v, dim):
    s = (v.reshape(len(v), -1, dim) ** 2).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = s / s.sum(-1, keepdims=True)
        t = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), np.where(p == 0, 0.0, np.nan))
    return np.exp(-t.sum(-1)) / s.shape[1]


def check(got, ref, what):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.nanmax(np.abs(got - ref)) if ref.size and not np.all(np.isnan(ref)) else 0.0
    print(f"{what}: max abs err {err:.3e}")
    assert np.allclose(got, ref, equal_nan=True), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ---- 1. one model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_atoms", [("anm", 20), ("gnm", 20), ("anm", 37), ("anm", 257), ("gnm", 37)])
def test_one_model(sc, kind, n_atoms):
    if n_atoms == 20:
        coord = sc.read_pdb_ca(ref_data("1l2y.pdb"))
        assert coord.array_length() == 20
    else:
        coord = synthetic_coord(n_atoms, 600 + n_atoms)
    dim, ntriv = (3, 6) if kind == "anm" else (1, 1)
    enm = sc.ANM(coord, sc.InvariantForceField(13.0)) if kind == "anm" else sc.GNM(coord, sc.InvariantForceField(10.0))
    _, v = enm.eigen()
    m = dim * n_atoms
    assert v.shape == (m, m)
    rs = np.random.RandomState(n_atoms)
    tail = (n_atoms, 3) if kind == "anm" else (n_atoms,)
    lists = {"default": None, "arange": np.arange(6, min(36, m)),
             "unsorted with a repeat": np.array([m - 1, 7, 12, 7, ntriv])}
    for q in (1, 3):
        d = rs.randn(q, *tail)
        for name, subset in lists.items():
            rows = np.arange(ntriv, m) if subset is None else subset
            tag = f"{kind} N = {n_atoms} q = {q} {name}"
            o = enm.overlap(d, mode_subset=subset)
            assert o.dtype == np.float64
            check(o, np_overlap(v[rows], d), tag + " overlap")
            assert np.array_equal(sc.nma.overlap(enm, d, subset), o)
            one = enm.overlap(d[1 if q > 1 else 0], mode_subset=subset)       # a single vector: (k,)
            assert one.shape == (len(rows),) and np.array_equal(one, o[1 if q > 1 else 0])
            if q == 1:
                check(enm.collectivity(mode_subset=subset), np_collectivity(v[rows], dim), tag + " collectivity")
        assert enm.overlap(d, mode_subset=[]).shape == (q, 0) and enm.overlap(d[0], mode_subset=[]).shape == (0,)
    assert enm.collectivity(mode_subset=[]).shape == (0,)
    kappa = enm.collectivity()
    assert np.all((kappa > 0) & (kappa <= 1 + 1e-12))
    with pytest.raises(IndexError):
        enm.overlap(d, mode_subset=[7, m])
    with pytest.raises(IndexError):
        enm.collectivity(mode_subset=[7, m])
    with pytest.raises(ValueError, match="Trivial modes"):
        enm.overlap(d, mode_subset=[ntriv - 1, 7])
    with pytest.raises(ValueError, match="Trivial modes"):
        enm.collectivity(mode_subset=[0])


# ---- 2. DeviceBatchSolver, full spectrum ---------------------------------------------------------------------------------------
N3, B3 = 171, 3


def test_batch_full_spectrum(sc, torch):
    coords = make_coords(N3, B3, seed=610)
    ff = sc.InvariantForceField(13.0)
    s, w, v = solved(sc, torch, coords, ff)
    m = 3 * N3
    rs = np.random.RandomState(611)
    kappa = s.collectivity()
    assert kappa.is_cuda and tuple(kappa.shape) == (B3, m) and kappa.dtype == torch.float64
    kappa = kappa.cpu().numpy()
    for b in range(B3):
        check(kappa[b], np_collectivity(v[b], 3), f"batch [{b}] collectivity")
    for q in (1, 5):
        d = rs.randn(B3, q, N3, 3)
        o = s.overlap(dev(torch, d))
        assert o.is_cuda and tuple(o.shape) == (B3, q, m) and o.dtype == torch.float64
        single = s.overlap(dev(torch, d[:, q - 1]))
        assert tuple(single.shape) == (B3, m) and torch.equal(single, o[:, q - 1])
        cum = sc.nma.cumulative_overlap(o)
        assert cum.is_cuda and tuple(cum.shape) == (B3, q, m)
        o, cum = o.cpu().numpy(), cum.cpu().numpy()
        for b in range(B3):
            check(o[b], np_overlap(v[b], d[b]), f"batch [{b}] q = {q} overlap")
        # completeness: the rows are an orthonormal basis
        total = np.sqrt((o**2).sum(-1))
        print("completeness: max |sqrt(sum O^2) - 1| =", np.abs(total - 1).max())
        assert np.allclose(total, 1.0)
        assert np.all(np.diff(cum, axis=-1) >= 0) and np.allclose(cum[..., -1], total)
    # another eigensolver path, the same meaning: structure 1 as an ANM.  An eigenvector is determined up to its sign, and
    # to about eps * lambda_max / gap; with gap > 1e-5 lambda_max that is ~1e-11, far inside the gate.
    anm = sc.ANM(coords[1], ff)
    gap = np.minimum(np.diff(w[1])[:-1], np.diff(w[1])[1:])             # of rows 1 .. m - 2
    unique = 1 + np.nonzero(gap > 1e-5 * w[1].max())[0]
    unique = unique[unique >= 7]
    assert len(unique) > 100
    o_anm = anm.overlap(d[1])                                          # rows 6 .. m - 1
    assert o_anm.shape == (5, m - 6)
    check(np.abs(o_anm[:, unique - 6]), np.abs(o[1][:, unique]), "batch [1] against nma.overlap of an ANM, |O|")
    check(anm.collectivity()[unique - 6], kappa[1][unique], "batch [1] against nma.collectivity of an ANM")


def test_batch_dim_1(sc, torch):
    coords = make_coords(N3, B3, seed=620)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(10.0), dim=1)
    d = np.random.RandomState(621).randn(B3, 2, N3)
    o = s.overlap(dev(torch, d)).cpu().numpy()
    kappa = s.collectivity().cpu().numpy()
    assert o.shape == (B3, 2, N3) and kappa.shape == (B3, N3)
    for b in range(B3):
        check(o[b], np_overlap(v[b], d[b]), f"dim 1 [{b}] overlap")
        check(kappa[b], np_collectivity(v[b], 1), f"dim 1 [{b}] collectivity")
    assert np.allclose(kappa[:, 0], 1.0)                               # the trivial mode of a GNM: every atom alike
    assert np.allclose(np.sqrt((o**2).sum(-1)), 1.0)
    with pytest.raises(ValueError, match=r"\(batch, N\) or \(batch, q, N\)"):
        s.overlap(dev(torch, np.zeros((B3, N3, 3))))


def test_batch_argument_errors_on_the_host(sc, torch):
    ff = sc.InvariantForceField(13.0)
    s = DeviceBatchSolver(N3, B3, ff)
    good = np.zeros((B3, N3, 3))
    for bad in (good[:2], np.zeros((B3, N3)), np.zeros((B3, 2, N3 + 1, 3)), np.zeros((B3, 3 * N3))):
        with pytest.raises(ValueError, match=r"\(batch, N, 3\) or \(batch, q, N, 3\)"):
            s.overlap(dev(torch, bad))
    for bad in (good, torch.from_numpy(good), dev(torch, good).float(), dev(torch, np.zeros((B3, 3, N3))).transpose(1, 2)):
        with pytest.raises(ValueError, match="contiguous CUDA float64"):
            s.overlap(bad)
    novec = DeviceBatchSolver(N3, B3, ff, want_vectors=False)
    with pytest.raises(ValueError, match="want_vectors=True"):
        novec.overlap(dev(torch, good))
    with pytest.raises(ValueError, match="want_vectors=True"):
        novec.collectivity()


# ---- 3. behind an index range and behind a value window ------------------------------------------------------------------------
def test_batch_behind_an_index_range(sc, torch):
    coords = make_coords(N3, B3, seed=630)
    d = np.random.RandomState(631).randn(B3, 2, N3, 3)
    s = DeviceBatchSolver(N3, B3, sc.InvariantForceField(13.0), subset_by_index=(0, 25))
    s.solve(dev(torch, coords))
    o = s.overlap(dev(torch, d))                        # enqueued straight behind the solve
    kappa = s.collectivity()
    s.finish()
    v = s.v.cpu().numpy()
    assert tuple(o.shape) == (B3, 2, 26) and tuple(kappa.shape) == (B3, 26)
    for b in range(B3):
        check(o[b].cpu().numpy(), np_overlap(v[b], d[b]), f"subset_by_index [{b}] overlap")
        check(kappa[b].cpu().numpy(), np_collectivity(v[b], 3), f"subset_by_index [{b}] collectivity")


def test_batch_behind_a_value_window_reads_the_counts_on_the_device(sc, torch):
    """Counts that differ, one that fills max_modes, one below it and one empty window: chosen on the CPU from LAPACK."""
    K = 24
    coords, mats, lam, (vl, vu), expected = window_case(N3, K, 3, batch=B3)
    assert len(set(expected)) == 3 and expected.max() == K and expected.min() == 0 and np.sum(expected < K) == 2
    d = np.random.RandomState(641).randn(B3, 2, N3, 3)
    s = DeviceBatchSolver(N3, B3, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    o = s.overlap(dev(torch, d))                        # enqueued straight behind the solve
    kappa = s.collectivity()
    s.finish()
    counts = s.counts.cpu().numpy()
    print("window counts", counts, "expected", expected)
    assert np.array_equal(counts, expected)
    v = s.v.cpu().numpy()
    o, kappa = o.cpu().numpy(), kappa.cpu().numpy()
    assert o.shape == (B3, 2, K) and kappa.shape == (B3, K)
    for b in range(B3):
        c = counts[b]
        assert np.all(np.isnan(o[b][:, c:])) and np.all(np.isnan(kappa[b][c:]))       # as the rows of w are
        assert np.all(np.isnan(s.w[b, c:].cpu().numpy()))
        if c == 0:
            assert np.all(np.isnan(o[b])) and np.all(np.isnan(kappa[b]))
            continue
        check(o[b][:, :c], np_overlap(v[b][:c], d[b]), f"window [{b}] count {c} overlap")
        check(kappa[b][:c], np_collectivity(v[b][:c], 3), f"window [{b}] count {c} collectivity")


# ---- 4. exact rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [20, 171])
def test_exact_rows(sc, torch, n_atoms):
    s, _, _ = solved(sc, torch, make_coords(n_atoms, 2, seed=650), sc.InvariantForceField(13.0))
    m = 3 * n_atoms
    rows = np.zeros((3, m))
    rows[0, 0::3] = 1.0 / np.sqrt(n_atoms)              # a rigid translation along x
    rows[1, 3 * 5 + 1] = 1.0                            # atom 5 alone, along y
    s.v[1, 6:9].copy_(torch.from_numpy(rows))           # (row 8: zeros)
    d = np.random.RandomState(651).randn(2, 3, n_atoms, 3)
    d[1, 1] = 0.0                                       # a zero displacement
    o = s.overlap(dev(torch, d)).cpu().numpy()
    kappa = s.collectivity().cpu().numpy()
    print("translation: kappa - 1 =", kappa[1, 6] - 1.0, " one atom: N kappa - 1 =", n_atoms * kappa[1, 7] - 1.0)
    assert abs(kappa[1, 6] - 1.0) <= 1e-12
    assert abs(kappa[1, 7] - 1.0 / n_atoms) <= 1e-12
    assert np.isnan(kappa[1, 8]) and np.sum(np.isnan(kappa)) == 1
    for j in (0, 2):
        unit = d[1, j] / np.linalg.norm(d[1, j])
        # one product and two norms of 3 N terms each: a few times 3 N eps / 2 ~ 3e-14 at N = 171
        assert np.isclose(o[1, j, 7], unit[5, 1], rtol=1e-13, atol=0)
        assert np.isclose(o[1, j, 6], unit[:, 0].sum() / np.sqrt(n_atoms), rtol=1e-12, atol=1e-13)
    assert np.all(np.isnan(o[1, 1]))                    # the zero displacement: that j only
    nan = np.isnan(o)
    assert np.all(nan[1, :, 8]) and nan.sum() == m + 2  # ... and the zero row, for every j
    assert not np.any(nan[0])


# ---- 5. placement, bit for bit ---------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_position_neighbours_or_q(sc, torch):
    ff = sc.HinsenForceField()                          # no cutoff: a NaN coordinate reaches the matrix
    x = synthetic_coord(N3, 660)
    others = make_coords(N3, 2, seed=661)
    s1, _, _ = solved(sc, torch, x[None], ff)
    s3, _, _ = solved(sc, torch, np.stack([x, others[0], others[1]]), ff)
    # the consumer's own property: the same eigenvectors alone, first of three and last of three
    s3.v[0].copy_(s1.v[0])
    s3.v[2].copy_(s1.v[0])
    rs = np.random.RandomState(662)
    d1 = rs.randn(1, 5, N3, 3)
    d3 = rs.randn(3, 5, N3, 3)
    d3[0] = d1[0]
    d3[2] = d1[0]
    o1, o3 = s1.overlap(dev(torch, d1)).cpu().numpy(), s3.overlap(dev(torch, d3)).cpu().numpy()
    k1, k3 = s1.collectivity().cpu().numpy(), s3.collectivity().cpu().numpy()
    assert np.array_equal(o1[0], o3[0]) and np.array_equal(o1[0], o3[2])
    assert np.array_equal(k1[0], k3[0]) and np.array_equal(k1[0], k3[2])
    # d_j alone against d_j as the third of five, and in the second group of four
    for j in (2, 4):
        assert np.array_equal(s1.overlap(dev(torch, d1[:, j])).cpu().numpy(), o1[:, j])
        assert np.array_equal(s3.overlap(dev(torch, d3[:, j: j + 1])).cpu().numpy()[:, 0], o3[:, j])
    # a repeated call
    assert np.array_equal(s3.overlap(dev(torch, d3)).cpu().numpy(), o3)
    assert np.array_equal(s3.collectivity().cpu().numpy(), k3)
    # a NaN coordinate in the middle structure
    coords = make_coords(N3, 3, seed=670)
    good, _, _ = solved(sc, torch, coords, ff)
    ref_o, ref_k = good.overlap(dev(torch, d3)).cpu().numpy(), good.collectivity().cpu().numpy()
    broken = coords.copy()
    broken[1, 7, 2] = np.nan
    bad = DeviceBatchSolver(N3, 3, ff)
    bad.solve(dev(torch, broken))
    got_o, got_k = bad.overlap(dev(torch, d3)), bad.collectivity()
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    got_o, got_k = got_o.cpu().numpy(), got_k.cpu().numpy()
    assert np.all(np.isnan(got_o[1])) and np.all(np.isnan(got_k[1]))
    for b in (0, 2):
        assert np.array_equal(got_o[b], ref_o[b]) and np.array_equal(got_k[b], ref_k[b])
        assert not np.any(np.isnan(got_o[b])) and not np.any(np.isnan(got_k[b]))


# ---- 6. RaggedBatchSolver --------------------------------------------------------------------------------------------------------
RAGGED = (20, 37, 171)


def _ragged(sc, torch, **kw):
    coords = [synthetic_coord(n, 680 + k) for k, n in enumerate(RAGGED)]
    s = RaggedBatchSolver(RAGGED, sc.InvariantForceField(13.0), **kw)
    s.solve(torch.from_numpy(np.concatenate(coords)).cuda().contiguous())
    s.finish()
    return s


def _own_plan_bits(sc, torch, s, b, d_b):
    """Structure b's eigenvectors in a plan of its own with the same slot order: its overlaps and collectivities there."""
    kw = dict(order=s.order)
    if s.subset is not None:
        kw["subset_by_index"] = s.subset
    alone = RaggedBatchSolver((RAGGED[b],), sc.InvariantForceField(13.0), **kw)
    assert alone.order == s.order and alone.v.shape[1:] == s.v.shape[1:]
    alone.w[0].copy_(s.w[b])
    alone.v[0].copy_(s.v[b])
    return alone.overlap(dev(torch, d_b))[0].cpu().numpy(), alone.collectivity()[0].cpu().numpy()


@pytest.mark.parametrize("subset_by_index", [None, (0, 25)])
def test_ragged_views_sizes_and_placement(sc, torch, subset_by_index):
    kw = {} if subset_by_index is None else dict(subset_by_index=subset_by_index)
    s = _ragged(sc, torch, **kw)
    assert s.order == 3 * max(RAGGED)
    per = s.results()
    freq = s.frequencies()
    total = sum(RAGGED)
    off = np.concatenate([[0], np.cumsum(RAGGED)])
    d = np.random.RandomState(690).randn(3, total, 3)
    o = s.overlap(dev(torch, d))
    one = s.overlap(dev(torch, d[1]))
    kappa = s.collectivity()
    assert len(o) == len(one) == len(kappa) == len(RAGGED)
    # another structure's displacement permuted: the packed vectors are read at the structure's own atom offset
    moved = d.copy()
    moved[:, off[0]: off[1]] = moved[:, off[0]: off[1]][:, ::-1]
    moved[:, off[2]: off[3]] = moved[:, off[2]: off[3]][:, ::-1]
    o_moved = s.overlap(dev(torch, moved))
    assert np.array_equal(o_moved[1].cpu().numpy(), o[1].cpu().numpy())
    assert not np.array_equal(o_moved[0].cpu().numpy(), o[0].cpu().numpy())
    for b, n in enumerate(RAGGED):
        v = per[b][1].cpu().numpy()
        rows = len(freq[b])
        assert v.shape == (rows, 3 * n) and rows == (3 * n if subset_by_index is None else 26)
        ob, kb = o[b].cpu().numpy(), kappa[b].cpu().numpy()
        assert ob.shape == (3, rows) and kb.shape == (rows,) and tuple(one[b].shape) == (rows,)
        assert np.array_equal(one[b].cpu().numpy(), ob[1])
        db = d[:, off[b]: off[b + 1]]
        tag = f"ragged {subset_by_index} [{b}] N = {n}"
        check(ob, np_overlap(v, db), tag + " overlap")
        check(kb, np_collectivity(v, 3), tag + " collectivity (N = the structure's own)")
        own_o, own_k = _own_plan_bits(sc, torch, s, b, db)
        assert np.array_equal(ob, own_o) and np.array_equal(kb, own_k), tag
    again = s.overlap(dev(torch, d))
    assert all(np.array_equal(a.cpu().numpy(), g.cpu().numpy()) for a, g in zip(again, o))


def test_ragged_dim_1_and_errors(sc, torch):
    sizes = (20, 37)
    ff = sc.InvariantForceField(10.0)
    coords = [synthetic_coord(n, 695 + k) for k, n in enumerate(sizes)]
    s = RaggedBatchSolver(sizes, ff, dim=1)
    s.solve(torch.from_numpy(np.concatenate(coords)).cuda().contiguous())
    s.finish()
    d = np.random.RandomState(696).randn(2, sum(sizes))
    o, kappa = s.overlap(dev(torch, d)), s.collectivity()
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b, n in enumerate(sizes):
        v = s.results()[b][1].cpu().numpy()
        check(o[b].cpu().numpy(), np_overlap(v, d[:, off[b]: off[b + 1]]), f"ragged dim 1 [{b}] overlap")
        check(kappa[b].cpu().numpy(), np_collectivity(v, 1), f"ragged dim 1 [{b}] collectivity")
    with pytest.raises(ValueError, match=r"\(S,\) or \(q, S\) with S = sum\(sizes\) = 57"):
        s.overlap(dev(torch, np.zeros((sum(sizes), 3))))
