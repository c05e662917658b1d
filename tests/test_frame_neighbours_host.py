"""
CPU-only checks of the frames' neighbour bits and of matrix-free neighbour-count clustering: the NumPy specification
(tests/frame_neighbours_model.py) against cluster_model.gromos on the model's own matrix, the epilogue's tile / lane -> word
map as a permutation, the two C entries' declarations, and every argument check of the Python layer, which happens before a
device is touched.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

from springcraft_amd import _hip
from tests import cluster_model as cm, ensemble_model as em, frame_neighbours_model as fm
from tests import test_cluster_host, test_rmsd_matrix_host

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_dev_frame_neighbours_f64": 10, "sc_dev_frame_neighbours_init_f64": 11}


# ---- the specification ---------------------------------------------------------------------------------------------------------
def _gromos_on_bits(bits, counts_valid, n, max_clusters=None):
    """The rounds of neighbour-count clustering on the packed bits alone."""
    near = fm.unpack(bits, n)
    alive = counts_valid.copy()
    labels = np.full(n, -1, dtype=np.int32)
    centres, sizes = [], []
    while alive.any() and (max_clusters is None or len(centres) < max_clusters):
        count = (near & alive[None, :]).sum(axis=1)
        count[~alive] = -1
        centre = int(np.argmax(count))
        members = near[centre] & alive
        labels[members] = len(centres)
        alive &= ~members
        centres.append(centre)
        sizes.append(int(members.sum()))
    return labels, np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32)


@pytest.mark.parametrize("n_frames, bad", [(20, ()), (70, ()), (70, (3, 66))])
def test_model_bits_give_the_clustering_of_the_matrix(n_frames, bad):
    frames, _ = cm.planted_frames(np.random.default_rng([n_frames, 5]), (n_frames // 3, n_frames // 3, n_frames - 2 * (n_frames // 3)),
                                  n_atoms=5)
    for b in bad:
        frames[b, 1, 2] = np.nan
    for cutoff in (0.0, 0.05, 1.0):
        bits, counts, valid, dist = fm.neighbours(frames, cutoff)
        assert bits.shape == (n_frames, fm.words_of(n_frames)) and bits.dtype == np.uint64
        near = fm.unpack(bits, n_frames)
        ok = fm.unpack(valid[None, :], n_frames)[0]
        assert np.array_equal(near, near.T) and np.array_equal(np.diag(near), ok) and not ok[list(bad)].any()
        assert not near[list(bad), :].any() and np.array_equal(counts, fm.popcounts(bits))      # (so the pad bits are 0)
        labels, centres, sizes, flag = cm.gromos(dist, cutoff)
        got = _gromos_on_bits(bits, ok, n_frames)
        assert flag == 0 and np.array_equal(got[0], labels) and np.array_equal(got[1], centres) and np.array_equal(got[2], sizes)
        got = _gromos_on_bits(bits, ok, n_frames, max_clusters=2)
        ref = cm.gromos(dist, cutoff, max_clusters=2)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_pack_and_unpack():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 130):
        near = rng.random((n, n)) < 0.3
        bits = fm.pack(near)
        assert bits.shape == (n, fm.words_of(n)) and np.array_equal(fm.unpack(bits, n), near)
        assert np.array_equal(fm.popcounts(bits), near.sum(axis=1))
        assert int(bits[0, 0]) & 1 == int(near[0, 0])
        if n == 65:
            assert all(int(bits[i, 1]) == int(near[i, 64]) for i in range(n))


# ---- the epilogue's lane map ------------------------------------------------------------------------------------------------------
def test_a_thread_slot_lands_on_its_own_column():
    stores = {}
    for tid in range(fm.THREADS):
        for j, r, i, c in fm.slots(tid):
            word, quarter, bit, storer = fm.ballot_store(tid, j, r)
            assert (word, 16 * quarter + bit) == (i, c)
            assert storer >> 6 == tid >> 6 and storer & 15 == 0          # lane 0 of the thread's 16-lane group
            stores.setdefault((word, quarter), set()).add((storer, j, r))
    # every uint16 of the 64-word tile has one storing lane and one (j, r); the halves of a word come from w and w ^ 4
    assert len(stores) == 64 * 4 and all(len(s) == 1 for s in stores.values())
    for word in range(64):
        waves = [next(iter(stores[(word, q)]))[0] >> 6 for q in range(4)]
        assert waves[0] == waves[1] and waves[2] == waves[3] and waves[0] ^ 4 == waves[2]


@pytest.mark.parametrize("n", [192, 129, 150])
def test_lane_map_is_a_permutation_of_the_bit_matrix(n):
    """Every (row, word, bit) of the matrix of a 3 x 3-tile triangle is produced exactly once, from its own pair."""
    words = fm.words_of(n)
    assert len(fm.tiles(n)) == 6
    seen = np.zeros((n, words, 64), dtype=np.int32)
    for tf, tg in fm.tiles(n):
        for row, word, bit, f, g in fm.tile_bits(tf, tg, n):
            seen[row, word, bit] += 1
            col = 64 * word + bit
            assert (row, col) in ((f, g), (g, f))
    assert (seen == 1).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entries_declared_exported_and_typed():
    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    assert {n for n in _hip.EXPORTED_SYMBOLS if "frame_neighbours" in n} == set(ENTRIES)
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name
    # the name sets the clustering and RMSD tests pin have not changed
    assert {n for n in _hip.EXPORTED_SYMBOLS if "cluster" in n} == set(test_cluster_host.ENTRIES)
    assert {n for n in _hip.EXPORTED_SYMBOLS if "rmsd" in n} == set(test_rmsd_matrix_host.ENTRIES)
    # a missing context is refused before anything else
    assert L.sc_dev_frame_neighbours_f64(None, None, 1, 1, None, 1, 1.0, None, None, None) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_frame_neighbours_init_f64(None, None, 1, 1, None, 1, 1.0, None, 0, None, None) == _hip.SC_ERR_INVALID_ARG


# ---- host-side argument checks: all raise before any device call (there is no device here) ---------------------------------------------
class _Stub:
    """An ensemble's host side alone: anything that would touch the device raises AssertionError."""

    def __init__(self, n_frames, n_atoms=5):
        from springcraft_amd.ensemble import Ensemble

        self.n_frames, self.n_atoms = n_frames, n_atoms
        self.cluster = Ensemble.cluster.__get__(self)
        self.neighbours = Ensemble.neighbours.__get__(self)

    def rmsd_matrix(self, **_):
        raise AssertionError("the matrix was asked for before the arguments were checked")

    def __getattr__(self, name):
        raise AssertionError(f"{name} was touched before the arguments were checked")


def test_neighbours_validation_needs_no_device():
    ens = _Stub(20)
    for cutoff in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="cutoff"):
            ens.neighbours(cutoff)
    with pytest.raises(ValueError, match="at most"):
        _Stub(262145).neighbours(1.0)
    with pytest.raises(ValueError, match="index range"):
        _Stub(20, 2 ** 31 // 3).neighbours(1.0)


def test_matrix_free_cluster_validation_needs_no_device():
    ens = _Stub(20)
    with pytest.raises(ValueError, match="matrix_free"):
        ens.cluster(method="kmedoids", k=3, matrix_free=True)
    for kw in (dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(), dict(cutoff=1.0, k=3),
               dict(cutoff=1.0, max_clusters=0), dict(cutoff=1.0, check_every=0), dict(cutoff=1.0, max_iter=5),
               dict(method="ward", cutoff=1.0)):
        with pytest.raises(ValueError):
            ens.cluster(matrix_free=True, **kw)
    with pytest.raises(ValueError, match="at most"):
        _Stub(262145).cluster(cutoff=1.0, matrix_free=True)
    with pytest.raises(ValueError, match="index range"):
        _Stub(20, 2 ** 31 // 3).cluster(cutoff=1.0, matrix_free=True)


def test_cluster_gromos_frames_validation_needs_no_device():
    import springcraft_amd as sc
    from springcraft_amd import cluster as cl

    assert sc.cluster_gromos_frames is cl.cluster_gromos_frames and "cluster_gromos_frames" in cl.__all__
    assert sc.FrameNeighbours is sc.ensemble.FrameNeighbours
    x = em.perturbed_ensemble(5, 4)
    for cutoff in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="cutoff"):
            sc.cluster_gromos_frames(x, cutoff)
    for bad in (np.zeros((4, 5)), np.zeros((4, 5, 2)), np.zeros(7), np.zeros((0, 5, 3)), np.zeros((4, 0, 3)),
                np.array([[["a", "b", "c"]]])):
        with pytest.raises(ValueError):
            sc.cluster_gromos_frames(bad, 1.0)
    for kw in (dict(max_clusters=0), dict(check_every=0), dict(weights=[1, 1, -1, 1, 1]), dict(weights=[0, 0, 0, 0, 0]),
               dict(weights=[1, 1, float("nan"), 1, 1])):
        with pytest.raises(ValueError):
            sc.cluster_gromos_frames(x, 1.0, **kw)
    with pytest.raises(IndexError, match="weights for 5 atoms"):
        sc.cluster_gromos_frames(x, 1.0, weights=np.ones(4))
    with pytest.raises(ValueError, match="at most"):
        sc.cluster_gromos_frames(np.zeros((cl.MAX_ITEMS + 1, 1, 3)), 1.0)
    with pytest.raises(ValueError, match="at most"):
        cl.check_frame_counts(cl.MAX_ITEMS + 1, 5)
    with pytest.raises(ValueError, match="index range"):
        cl.check_frame_counts(20, 2 ** 31 // 3)
    cl.check_frame_counts(cl.MAX_ITEMS, 2000)
