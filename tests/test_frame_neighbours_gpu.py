"""
GPU checks of the frames' neighbour bits (csrc/rmsd_matrix.hip's bit epilogue, ``Ensemble.neighbours``) and of matrix-free
neighbour-count clustering (``Ensemble.cluster(matrix_free=True)``, ``cluster_gromos_frames``).

Bits against the matrix.  ``neighbours(cutoff).dense()`` is compared on the device with ``rmsd_matrix() <= cutoff``, the
diagonal forced true, on every pair outside the guard band ``|d - cutoff| <= 64 eps (G_f + G_g) / (W cutoff)``: the value is
``sqrt(((G_f + G_g) - 2 lambda) / W)``, the difference carries a rounding error of the order eps (G_f + G_g) / W, and the root
divides it by 2 sqrt(.) = 2 cutoff at the cutoff.  With ``squared`` there is no root and the band is ``64 eps (G_f + G_g) / W``.
A band of width 0 or one that is not a number (G 0, and for the root cutoff 0: one atom, fitted, where every value is an exact
0 without any rounding) holds no pair.  The cutoff is the median of the matrix'
entries (NumPy's: the mean of the middle two of an even count), so for an odd M one pair and its mirror image sit on the
cutoff itself and in the band: at most 2 of M (M - 1) >= 3906 ordered pairs of distinct frames, 0.05 %.  The share of those
pairs inside the band must be at most 1 %.  Both sides come from one value function, so the number of differing bits over ALL
pairs, the band included, is printed too, and is expected to be 0.

Clustering compares only, so labels, representatives and sizes must EQUAL those of the two-step ``cluster()`` and of
``cluster_model.gromos`` on the device's matrix, read back.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from springcraft_amd import _hip
from tests import cluster_model as cm, frame_neighbours_model as fm, rmsd_matrix_model as rm

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FRAMES = [1, 2, 63, 64, 65, 127, 128, 129, 200]      # the tile edges; 129 and 200: off-diagonal tiles with a partial last one
ATOMS = [1, 3, 8, 9, 50]                             # on and off the staged group of 8 atoms
MAX_FRAMES = max(FRAMES)


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def random_frames(n_atoms):
    frames = rm.case_frames(n_atoms, MAX_FRAMES)
    frames.setflags(write=False)
    return frames


def moments(torch, ens, fit):
    """(G (M,), W) of the frames of ``ens`` on the device, as the definition has them."""
    x = ens.frames
    w = torch.ones(ens.n_atoms, dtype=torch.float64, device=x.device) if ens._w is None else ens._w
    wsum = w.sum()
    if fit:
        c = (w[None, :, None] * x).sum(dim=1) / wsum
    else:
        c = ((w[:, None] * x[0]).sum(dim=0) / wsum)[None, :].expand(ens.n_frames, 3)
    g = (w[None, :] * ((x - c[:, None, :]) ** 2).sum(dim=2)).sum(dim=1)
    return g, wsum


def check_bits(sc, torch, frames, weights, fit, squared, label):
    """The whole comparison of one input; returns (ens, cutoff, the FrameNeighbours)."""
    m = len(frames)
    ens = sc.Ensemble(frames, weights=weights)
    d = ens.rmsd_matrix(fit=fit, squared=squared)
    cutoff = float(np.median(d.cpu().numpy()))
    nb = ens.neighbours(cutoff, fit=fit, squared=squared)
    words = (m + 63) // 64
    assert nb.bits.is_cuda and nb.bits.dtype == torch.int64 and tuple(nb.bits.shape) == (m, words)
    assert nb.counts.dtype == torch.int32 and tuple(nb.counts.shape) == (m,)
    assert nb.valid.dtype == torch.int64 and tuple(nb.valid.shape) == (words,)
    dense = nb.dense()
    assert dense.dtype == torch.bool and tuple(dense.shape) == (m, m)

    eye = torch.eye(m, dtype=torch.bool, device=d.device)
    g, wsum = moments(torch, ens, fit)
    band = 64 * EPS * (g[:, None] + g[None, :]) / (wsum if squared else wsum * cutoff)
    in_band = ((d - cutoff).abs() <= band) & (band > 0) & ~eye
    share = float(in_band.sum()) / max(1, m * (m - 1))
    expect = (d <= cutoff) | eye
    differ = int((dense != expect).sum())
    print(f"{label}: cutoff {cutoff:.6g}, {int(in_band.sum())} of {m * (m - 1)} pairs in the band ({100 * share:.3f} %), "
          f"{differ} bits differ from rmsd_matrix() <= cutoff over all pairs")
    assert share <= 0.01
    assert torch.equal(dense | in_band, expect | in_band)

    # the structure: counts, symmetry, the diagonal, the pad bits, validity, repeatability
    host = nb.bits.cpu().numpy()
    assert np.array_equal(fm.unpack(host, m), dense.cpu().numpy())
    assert np.array_equal(nb.counts.cpu().numpy(), fm.popcounts(host))               # (pad bits would be counted here)
    assert np.array_equal(nb.counts.cpu().numpy(), dense.sum(dim=1).cpu().numpy())
    assert torch.equal(dense, dense.T) and bool(torch.diagonal(dense).all())
    assert np.array_equal(fm.unpack(nb.valid.cpu().numpy()[None, :], 64 * words)[0], np.arange(64 * words) < m)
    again = ens.neighbours(cutoff, fit=fit, squared=squared)
    assert torch.equal(again.bits, nb.bits) and torch.equal(again.counts, nb.counts) and torch.equal(again.valid, nb.valid)
    return ens, cutoff, nb


# ---- 1. bits against the matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", ATOMS)
@pytest.mark.parametrize("n_frames", FRAMES)
def test_bits_equal_the_thresholded_matrix(sc, torch, n_frames, n_atoms):
    check_bits(sc, torch, random_frames(n_atoms)[:n_frames], None, True, False, f"M={n_frames} N={n_atoms}")


# (a single atom cannot carry a zero weight beside a positive sum: the weights variant starts at three atoms, two weighted)
@pytest.mark.parametrize("variant, n_atoms", [(v, a) for v in ("nofit", "squared", "weights") for a in ATOMS
                                              if not (v == "weights" and a == 1)])
@pytest.mark.parametrize("n_frames", FRAMES)
def test_bits_of_the_variants(sc, torch, n_frames, n_atoms, variant):
    w = rm.case_weights(n_atoms, True) if variant == "weights" else None
    assert w is None or (w == 0).any()
    check_bits(sc, torch, random_frames(n_atoms)[:n_frames], w, variant != "nofit", variant == "squared",
               f"{variant} M={n_frames} N={n_atoms}")


def test_cutoff_zero_and_above_the_maximum(sc, torch):
    frames = np.array(random_frames(9)[:130])
    frames[77] = frames[3]                                  # an exact duplicate across two tiles
    ens = sc.Ensemble(frames)
    d = ens.rmsd_matrix()
    eye = torch.eye(130, dtype=torch.bool, device=d.device)
    nb = ens.neighbours(0.0)
    assert torch.equal(nb.dense(), (d <= 0.0) | eye) and int(nb.counts[3]) >= 1
    nb = ens.neighbours(float(d.max()))
    assert bool(nb.dense().all()) and bool((nb.counts == 130).all())


# ---- 2. independence ------------------------------------------------------------------------------------------------------------------
def test_a_subset_alone_gives_the_sub_matrix(sc, torch):
    frames = random_frames(9)
    ens, cutoff, full = check_bits(sc, torch, frames, None, True, False, "independence, all frames")
    keep = np.sort(np.random.default_rng(4).choice(MAX_FRAMES, size=70, replace=False))
    sub = sc.Ensemble(frames[keep]).neighbours(cutoff)
    idx = torch.from_numpy(keep).to(full.bits.device)
    assert torch.equal(sub.dense(), full.dense()[idx][:, idx])
    assert np.array_equal(sub.counts.cpu().numpy(), fm.popcounts(sub.bits.cpu().numpy()))


# ---- 3. non-finite frames -------------------------------------------------------------------------------------------------------------
def test_non_finite_frames_have_no_neighbours(sc, torch):
    m, bad = MAX_FRAMES, [5, 130]                           # one in tile 0, one in tile 2
    clean = random_frames(9)
    frames = np.array(clean)
    frames[5, 2, 1] = np.nan
    frames[130, 7, 0] = np.inf
    ens = sc.Ensemble(frames)
    cutoff = float(np.nanmedian(ens.rmsd_matrix().cpu().numpy()))
    nb = ens.neighbours(cutoff)
    dense = nb.dense().cpu().numpy()
    assert not dense[bad, :].any() and not dense[:, bad].any() and (nb.counts.cpu().numpy()[bad] == 0).all()
    valid = fm.unpack(nb.valid.cpu().numpy()[None, :], 64 * ((m + 63) // 64))[0]
    expect_valid = np.arange(len(valid)) < m
    expect_valid[bad] = False
    assert np.array_equal(valid, expect_valid)
    # every other bit is the run's with those frames replaced by finite ones
    keep = np.array([i for i in range(m) if i not in bad])
    ref = sc.Ensemble(clean).neighbours(cutoff).dense().cpu().numpy()
    assert np.array_equal(dense[np.ix_(keep, keep)], ref[np.ix_(keep, keep)])
    assert np.array_equal(nb.counts.cpu().numpy(), fm.popcounts(nb.bits.cpu().numpy()))
    r = ens.cluster(cutoff=cutoff, matrix_free=True)
    two = ens.cluster(cutoff=cutoff)
    labels = r.labels.cpu().numpy()
    assert r.flag == 0 and (labels[bad] == -1).all() and (labels[keep] >= 0).all()
    assert torch.equal(r.labels, two.labels) and torch.equal(r.representatives, two.representatives)
    assert torch.equal(r.sizes, two.sizes) and int(r.sizes.sum()) == m - 2


# ---- 4. clustering ------------------------------------------------------------------------------------------------------------------
def _group_sizes(n, groups):
    base = [n // groups] * groups
    for g in range(n - sum(base)):
        base[g] += 1
    return tuple(base)


@functools.lru_cache(maxsize=None)
def planted(n, groups):
    frames, lab = cm.planted_frames(np.random.default_rng([n, groups, 2]), _group_sizes(n, groups), n_atoms=8, noise=0.02,
                                    separation=4.0)
    frames.setflags(write=False)
    return frames, lab


@pytest.mark.parametrize("n, groups", [(65, 3), (200, 7)])
def test_matrix_free_clustering_equals_the_two_step(sc, torch, n, groups):
    frames, lab = planted(n, groups)
    ens = sc.Ensemble(frames)
    d = ens.rmsd_matrix()
    same = torch.from_numpy(lab[:, None] == lab[None, :]).to(d.device)
    assert not bool(((d >= 0.5) & (d <= 2.0)).any())                          # no pair near the cutoff
    assert float(d[same].max()) <= 0.3 and float(d[~same].min()) >= 3.0
    host = d.cpu().numpy()
    labels, centres, sizes, flag = cm.gromos(host, 1.0)
    assert flag == 0 and len(centres) == groups and cm.same_partition(labels, lab)
    two = ens.cluster("gromos", cutoff=1.0)
    free = ens.cluster("gromos", cutoff=1.0, matrix_free=True)
    assert free.method == "gromos" and free.labels.is_cuda and free.labels.dtype == torch.int32
    for r in (two, free):
        assert r.flag == 0 and r.n_clusters == groups
        assert np.array_equal(r.labels.cpu().numpy(), labels) and np.array_equal(r.representatives.cpu().numpy(), centres)
        assert np.array_equal(r.sizes.cpu().numpy(), sizes)
    # NumPy in, NumPy out
    h = sc.cluster_gromos_frames(np.array(frames), 1.0)
    assert isinstance(h.labels, np.ndarray) and isinstance(h.representatives, np.ndarray) and isinstance(h.members(0), np.ndarray)
    assert np.array_equal(h.labels, labels) and np.array_equal(h.representatives, centres) and np.array_equal(h.sizes, sizes)
    assert h.labels.dtype == np.int32 and h.n_clusters == groups
    # max_clusters: the rounds are enqueued, nothing is read, what is left over keeps -1
    part = ens.cluster("gromos", cutoff=1.0, matrix_free=True, max_clusters=2)
    assert part.status_reads == 0
    ref = cm.gromos(host, 1.0, max_clusters=2)
    assert part.n_clusters == 2 and part.status_reads == 1
    got = part.labels.cpu().numpy()
    assert np.array_equal(got, ref[0]) and (got == -1).sum() == n - int(ref[2].sum()) > 0
    assert np.array_equal(part.representatives.cpu().numpy(), ref[1]) and np.array_equal(part.sizes.cpu().numpy(), ref[2])
    # check_every does not matter
    runs = [ens.cluster("gromos", cutoff=1.0, matrix_free=True, check_every=ce) for ce in (1, 32)]
    assert runs[0].status_reads == groups and runs[1].status_reads == 1
    for r in runs:
        assert torch.equal(r.labels, free.labels) and torch.equal(r.representatives, free.representatives)
        assert torch.equal(r.sizes, free.sizes)


def test_matrix_free_variants_equal_the_two_step(sc, torch):
    frames = random_frames(9)
    w = rm.case_weights(9, True)
    for fit, squared, weights in ((False, False, None), (True, True, None), (True, False, w)):
        ens = sc.Ensemble(frames, weights=weights)
        cutoff = 0.6 * float(np.median(ens.rmsd_matrix(fit=fit, squared=squared).cpu().numpy()))
        two = ens.cluster(cutoff=cutoff, fit=fit, squared=squared)
        free = ens.cluster(cutoff=cutoff, fit=fit, squared=squared, matrix_free=True)
        nb = ens.neighbours(cutoff, fit=fit, squared=squared)
        differ = int((nb.dense() != ((ens.rmsd_matrix(fit=fit, squared=squared) <= cutoff)
                                     | torch.eye(MAX_FRAMES, dtype=torch.bool, device=nb.bits.device))).sum())
        print(f"fit={fit} squared={squared} weights={weights is not None}: {two.n_clusters} clusters, {differ} bits differ")
        if differ == 0:                 # (a pair on the cutoff may round either way; then the partitions need not agree)
            assert torch.equal(free.labels, two.labels) and torch.equal(free.representatives, two.representatives)
            assert torch.equal(free.sizes, two.sizes)
        assert int(free.sizes.sum()) == MAX_FRAMES and free.flag == 0


# ---- 5. the C entries' range checks ------------------------------------------------------------------------------------------------
def test_entries_refuse_what_is_out_of_range(sc, torch):
    L, bad = _hip.lib(), _hip.SC_ERR_INVALID_ARG
    ctx = _hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n, atoms = 10, 4
    size = L.sc_cluster_workspace(n, 0)
    ws = torch.empty((size,), dtype=torch.uint8, device="cuda")
    x = torch.zeros((n, atoms, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((n,), dtype=torch.int64, device="cuda")
    p, w, o, h = C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), ctx.handle
    for args in ((p, 0, atoms, None, 1, 1.0, o, o, o), (p, n, 0, None, 1, 1.0, o, o, o), (p, 262145, atoms, None, 1, 1.0, o, o, o),
                 (p, n, 2 ** 31 // 3, None, 1, 1.0, o, o, o), (p, n, atoms, None, 4, 1.0, o, o, o),
                 (p, n, atoms, None, 1, -1.0, o, o, o), (p, n, atoms, None, 1, float("nan"), o, o, o),
                 (p, n, atoms, None, 1, float("inf"), o, o, o), (None, n, atoms, None, 1, 1.0, o, o, o),
                 (p, n, atoms, None, 1, 1.0, None, o, o), (p, n, atoms, None, 1, 1.0, o, None, o),
                 (p, n, atoms, None, 1, 1.0, o, o, None)):
        assert L.sc_dev_frame_neighbours_f64(h, *args) == bad, args
    for args in ((p, 0, atoms, None, 1, 1.0, w, size, o, o), (p, 262145, atoms, None, 1, 1.0, w, size, o, o),
                 (p, n, atoms, None, 8, 1.0, w, size, o, o), (p, n, atoms, None, 1, -1.0, w, size, o, o),
                 (p, n, atoms, None, 1, float("nan"), w, size, o, o), (p, n, atoms, None, 1, 1.0, None, size, o, o),
                 (p, n, atoms, None, 1, 1.0, w, 64, o, o), (None, n, atoms, None, 1, 1.0, w, size, o, o),
                 (p, n, atoms, None, 1, 1.0, w, size, None, o), (p, n, atoms, None, 1, 1.0, w, size, o, None)):
        assert L.sc_dev_frame_neighbours_init_f64(h, *args) == bad, args
    ctx.synchronize()
    # the context works afterwards
    assert sc.cluster_gromos_frames(np.array(random_frames(3)[:10]), 100.0).n_clusters == 1
