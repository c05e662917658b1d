"""
GPU checks of the clustering (csrc/cluster.hip, springcraft_amd/cluster.py) against the NumPy specification of
tests/cluster_model.py, evaluated on the device's own matrix, read back.

Neighbour-count clustering only compares, so labels, centres and sizes must EQUAL the specification's on any input.
k-medoids adds: on dyadic matrices (multiples of 2^-10 below 8) every sum is exact in any order, so medoids, labels, the
total-deviation history and the iteration count must equal the specification's too.  On real RMSD matrices the device's
sums have their own fixed order; there the result is checked by what it promises: the planted partition, a strictly
decreasing total deviation, and local optimality -- with the specification's longdouble delta at the device's final medoids
no delta is below ``-2 M eps sum_j ds[j]``, the rounding bound of an M-term sum of terms bounded by ds in any order.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from springcraft_amd import _hip
from tests import cluster_model as cm

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 63, 64, 65, 130, 200]          # the 64-bit word edges and a partial last word
KMED_SIZES = [2, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def dyadic(n, duplicates=False):
    d = cm.dyadic_matrix(np.random.default_rng([n, 17]), n)
    if duplicates and n >= 2:
        for a in range(0, n - 1, 5):          # planted duplicates: pairs, and one triple where there is room
            d[a, a + 1] = d[a + 1, a] = 0.0
        if n >= 8:
            d[5, 7] = d[7, 5] = d[6, 7] = d[7, 6] = 0.0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def frames_of(n, seed=3):
    frames, planted = cm.planted_frames(np.random.default_rng([n, seed]), _group_sizes(n, 7), n_atoms=8)
    frames.setflags(write=False)
    return frames, planted


def _group_sizes(n, groups):
    groups = min(groups, n)
    base = [n // groups] * groups
    for g in range(n - sum(base)):
        base[g] += 1
    return tuple(base)


def _assert_gromos(result, dist, cutoff, max_clusters=None):
    labels, centres, sizes, flag = cm.gromos(dist, cutoff, max_clusters)
    assert result.flag == flag and result.n_clusters == len(centres)
    assert result.labels.dtype == np.int32 and result.representatives.dtype == np.int32 and result.sizes.dtype == np.int32
    assert np.array_equal(result.labels, labels)
    assert np.array_equal(result.representatives, centres) and np.array_equal(result.sizes, sizes)
    return len(centres)


# ---- neighbour count: exact equality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_gromos_dyadic_equals_the_specification(sc, n):
    d = dyadic(n)
    for cutoff in (1.0, 3.0):                                    # mid values
        _assert_gromos(sc.cluster_gromos(d, cutoff), d, cutoff)
    assert _assert_gromos(sc.cluster_gromos(d, 8.0), d, 8.0) == 1   # above the maximum: one round
    dup = dyadic(n, True)
    made = _assert_gromos(sc.cluster_gromos(dup, 0.0), dup, 0.0)    # duplicates only
    assert made < n or n == 1
    r = sc.cluster_gromos(d, 1.0)
    assert isinstance(r.labels, np.ndarray) and r.iterations is None and r.total_deviation is None
    assert sorted(np.concatenate([r.members(c) for c in range(r.n_clusters)]).tolist()) == list(range(n))


@pytest.mark.parametrize("n", SIZES)
def test_gromos_on_a_real_rmsd_matrix(sc, torch, n):
    frames, _ = frames_of(n)
    ens = sc.Ensemble(frames)
    dist = ens.rmsd_matrix()
    host = dist.cpu().numpy()
    for cutoff in ({0.0, float(np.median(host)), float(host.max()) * 0.25}):
        r = ens.cluster("gromos", cutoff=cutoff)
        assert r.labels.is_cuda and r.labels.dtype == torch.int32
        labels, centres, sizes, _ = cm.gromos(host, cutoff)
        assert np.array_equal(r.labels.cpu().numpy(), labels) and np.array_equal(r.representatives.cpu().numpy(), centres)
        assert np.array_equal(r.sizes.cpu().numpy(), sizes) and r.n_clusters == len(centres)
        assert np.array_equal(r.members(0).cpu().numpy(), np.flatnonzero(labels == 0))


def test_gromos_singletons_cross_the_chunks_and_check_every_does_not_matter(sc):
    d = dyadic(130)
    runs = {ce: sc.cluster_gromos(d, 0.0, check_every=ce) for ce in (1, 7, 32)}     # no duplicates: 130 rounds
    assert _assert_gromos(runs[32], d, 0.0) == 130 and runs[32].representatives.tolist() == list(range(130))
    assert (runs[1].status_reads, runs[7].status_reads, runs[32].status_reads) == (130, 19, 5)
    for cutoff, n in ((1.0, 130), (2.0, 200)):
        d = dyadic(n)
        runs = [sc.cluster_gromos(d, cutoff, check_every=ce) for ce in (1, 7, 32, 32)]
        for r in runs[1:]:
            assert np.array_equal(r.labels, runs[0].labels) and np.array_equal(r.sizes, runs[0].sizes)
            assert np.array_equal(r.representatives, runs[0].representatives)


def test_gromos_max_clusters_reads_nothing(sc, torch):
    d = dyadic(200)
    t = torch.from_numpy(np.array(d)).cuda()
    r = sc.cluster_gromos(t, 1.0, max_clusters=3)
    assert r.status_reads == 0                                    # the call returned without a read: nothing waited
    labels, centres, sizes, _ = cm.gromos(d, 1.0, max_clusters=3)
    assert r.n_clusters == 3 and r.status_reads == 1
    assert np.array_equal(r.labels.cpu().numpy(), labels) and (labels == -1).any()
    assert np.array_equal(r.representatives.cpu().numpy(), centres) and np.array_equal(r.sizes.cpu().numpy(), sizes)
    # more clusters allowed than there are: the rounds after the last one do nothing
    r = sc.cluster_gromos(t, 3.0, max_clusters=150)
    full = cm.gromos(d, 3.0)
    assert r.n_clusters == len(full[1]) < 150 and np.array_equal(r.labels.cpu().numpy(), full[0])


def test_gromos_designed_ties_go_to_the_lower_index(sc):
    # items 3 and 9 both see three others, every other item fewer: 3 wins; then 9 is the largest of the rest
    n = 70
    d = np.full((n, n), 5.0)
    np.fill_diagonal(d, 0.0)
    for centre, others in ((9, (20, 40, 69)), (3, (10, 30, 65))):
        for o in others:
            d[centre, o] = d[o, centre] = 1.0
    r = sc.cluster_gromos(d, 1.0)
    assert r.representatives[:2].tolist() == [3, 9] and r.sizes[:3].tolist() == [4, 4, 1]
    assert r.representatives[2:].tolist() == [i for i in range(n) if i not in (3, 9, 10, 30, 65, 20, 40, 69)]
    _assert_gromos(r, d, 1.0)


@pytest.mark.parametrize("bad", [(5,), (0, 64)])
def test_gromos_nan_frames_are_left_out(sc, bad):
    frames = np.array(frames_of(130)[0])
    for b in bad:
        frames[b, 2, 1] = np.nan
    ens = sc.Ensemble(frames)
    host = ens.rmsd_matrix().cpu().numpy()
    cutoff = float(np.nanmedian(host))
    r = ens.cluster("gromos", cutoff=cutoff)
    keep = np.array([i for i in range(130) if i not in bad])
    sub = cm.gromos(host[np.ix_(keep, keep)], cutoff)
    labels = r.labels.cpu().numpy()
    assert (labels[list(bad)] == -1).all() and np.array_equal(labels[keep], sub[0]) and r.flag == 0
    assert np.array_equal(r.representatives.cpu().numpy(), keep[sub[1]]) and np.array_equal(r.sizes.cpu().numpy(), sub[2])
    k = ens.cluster("kmedoids", k=3)
    ksub = cm.kmedoids(host[np.ix_(keep, keep)], 3)
    assert (k.labels.cpu().numpy()[list(bad)] == -1).all() and k.sizes.cpu().numpy().sum() == len(keep)
    assert cm.same_partition(k.labels.cpu().numpy()[keep], ksub["labels"])


def test_nan_between_valid_items_sets_the_flag(sc):
    d = np.array(dyadic(65))
    d[3, 64] = np.nan
    r = sc.cluster_gromos(d, 2.0)
    assert r.flag == 1 and r.n_clusters == 0 and (r.labels == -1).all() and len(r.representatives) == 0 and len(r.sizes) == 0
    r = sc.cluster_kmedoids(d, 3)
    assert r.flag == 1 and r.n_clusters == 0 and (r.labels == -1).all() and len(r.representatives) == 0
    assert len(r.total_deviation) == 0


# ---- k-medoids on dyadic matrices: exact equality -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kmed_reference(n, k):
    return cm.kmedoids(dyadic(n), k)


def _assert_kmedoids(result, ref):
    assert result.flag == ref["flag"] and result.n_clusters == len(ref["medoids"])
    assert np.array_equal(result.representatives, ref["medoids"]) and np.array_equal(result.labels, ref["labels"])
    assert np.array_equal(result.sizes, ref["sizes"])
    assert result.iterations == ref["iterations"] and result.converged == ref["converged"]
    assert np.array_equal(result.total_deviation, ref["td"])


@pytest.mark.parametrize("n, k", [(n, k) for n in KMED_SIZES for k in sorted({1, 2, 3, 7, n}) if k <= n])
def test_kmedoids_dyadic_equals_the_specification(sc, n, k):
    r = sc.cluster_kmedoids(dyadic(n), k)
    ref = kmed_reference(n, k)
    assert r.labels.dtype == np.int32 and r.total_deviation.dtype == np.float64
    _assert_kmedoids(r, ref)
    assert np.all(np.diff(r.total_deviation) < 0)


def test_kmedoids_check_every_and_repeat_give_the_same_bits(sc):
    d = dyadic(130)
    ref = kmed_reference(130, 7)
    assert ref["iterations"] >= 2
    for ce in (1, 3, 100):
        _assert_kmedoids(sc.cluster_kmedoids(d, 7, check_every=ce), ref)


def test_kmedoids_max_iter_runs_out_without_raising(sc):
    d = dyadic(130)
    ref = kmed_reference(130, 7)
    assert ref["iterations"] >= 2                                    # the input needs more than one swap
    r = sc.cluster_kmedoids(d, 7, max_iter=1)
    assert r.converged is False and r.iterations == 1 and len(r.total_deviation) == 2
    assert np.array_equal(r.total_deviation, ref["td"][:2])
    _assert_kmedoids(r, cm.kmedoids(d, 7, max_iter=1))


# ---- k-medoids on real RMSD matrices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 7])
def test_kmedoids_on_a_real_rmsd_matrix(sc, k):
    n = 130
    frames, planted = cm.planted_frames(np.random.default_rng([n, k]), _group_sizes(n, k), n_atoms=8, noise=0.05)
    ens = sc.Ensemble(frames)
    host = ens.rmsd_matrix().cpu().numpy()
    r = ens.cluster("kmedoids", k=k)
    labels, medoids, td = r.labels.cpu().numpy(), r.representatives.cpu().numpy(), r.total_deviation.cpu().numpy()
    assert r.converged and r.n_clusters == k and cm.same_partition(labels, planted)
    assert np.all(np.diff(td) < 0) and len(td) == r.iterations + 1
    valid = np.ones(n, dtype=bool)
    nearest, dn, ds = cm.assign(host, medoids.tolist(), valid)
    assert np.array_equal(nearest, labels) and np.array_equal(np.bincount(labels, minlength=k), r.sizes.cpu().numpy())
    assert abs(td[-1] - dn.sum()) <= 2 * n * EPS * dn.sum()
    # local optimality inside the rounding bound of an M-term sum
    delta = cm.swap_deltas(host, medoids.tolist(), valid, dtype=np.longdouble)
    gate = 2 * n * EPS * ds.sum()
    worst = max(0.0, float(-delta.min()))
    print(f"k-medoids M={n} k={k}: {r.iterations} swaps, most negative delta {worst:.3e} / gate {gate:.3e} = {worst / gate:.3f}")
    assert worst <= gate


# ---- forms and limits --------------------------------------------------------------------------------------------------------------
def test_both_forms_give_identical_bits(sc, monkeypatch):
    frames, _ = frames_of(130)
    host = sc.rmsd_matrix(np.array(frames))
    first = None
    for form in ("lds", "stream", "lds", "stream"):                 # (the repeats: two calls agree bit for bit)
        monkeypatch.setenv("SPRINGCRAFT_CLUSTER_FORM", form)
        assert _hip.lib().sc_cluster_form(130, 7) == (0 if form == "lds" else 1)
        r = sc.cluster_kmedoids(host, 7)
        first = first or r
        assert np.array_equal(r.labels, first.labels) and np.array_equal(r.representatives, first.representatives)
        assert np.array_equal(r.total_deviation, first.total_deviation) and r.iterations == first.iterations
    d = dyadic(130)
    for form in ("lds", "stream"):
        monkeypatch.setenv("SPRINGCRAFT_CLUSTER_FORM", form)
        _assert_kmedoids(sc.cluster_kmedoids(d, 7), kmed_reference(130, 7))


def test_entries_refuse_what_is_out_of_range(sc, torch):
    L, bad = _hip.lib(), _hip.SC_ERR_INVALID_ARG
    ctx = _hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n, k = 10, 3
    ws = torch.empty((max(L.sc_cluster_workspace(n, 0), L.sc_cluster_workspace(n, k)),), dtype=torch.uint8, device="cuda")
    buf = torch.zeros((n * n,), dtype=torch.float64, device="cuda")
    ints = torch.zeros((n,), dtype=torch.int32, device="cuda")
    p, w, i, size = C.c_void_p(buf.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(ints.data_ptr()), ws.numel()
    h = ctx.handle
    for args in ((p, 0, 1.0, w, size, i, i), (p, 262145, 1.0, w, size, i, i), (p, n, -1.0, w, size, i, i),
                 (p, n, float("nan"), w, size, i, i), (p, n, float("inf"), w, size, i, i), (p, n, 1.0, None, size, i, i),
                 (p, n, 1.0, w, 64, i, i), (None, n, 1.0, w, size, i, i), (p, n, 1.0, w, size, None, i),
                 (p, n, 1.0, w, size, i, None)):
        assert L.sc_dev_cluster_gromos_init_f64(h, *args) == bad, args
    for args in ((n, 0, n, w, size, i, i, i, i), (n, n + 1, n, w, size, i, i, i, i), (n, 1, 0, w, size, i, i, i, i),
                 (n, 1, n + 1, w, size, i, i, i, i), (n, 1, n, w, 64, i, i, i, i), (n, 1, n, w, size, i, None, i, i)):
        assert L.sc_dev_cluster_gromos_rounds(h, *args) == bad, args
    for args in ((p, n, 0, w, size, i, i, i, p, 4, i), (p, n, n + 1, w, size, i, i, i, p, 4, i), (p, n, k, w, 64, i, i, i, p, 4, i),
                 (p, n, k, w, size, i, i, i, p, 0, i), (p, n, k, w, size, i, i, i, None, 4, i), (None, n, k, w, size, i, i, i, p, 4, i)):
        assert L.sc_dev_cluster_kmedoids_init_f64(h, *args) == bad, args
    for args in ((p, n, k, 0, w, size, i, i, i, p, 4, i), (p, n, k, 65537, w, size, i, i, i, p, 4, i),
                 (p, n, 0, 1, w, size, i, i, i, p, 4, i), (p, n, k, 1, w, size, i, i, i, p, 4, None)):
        assert L.sc_dev_cluster_kmedoids_swaps_f64(h, *args) == bad, args
    ctx.synchronize()
    # the context works afterwards
    assert sc.cluster_gromos(np.array(dyadic(10)), 8.0).n_clusters == 1


# ---- Ensemble.cluster -----------------------------------------------------------------------------------------------------------------
def test_ensemble_cluster(sc, torch):
    frames, _ = frames_of(65)
    ens = sc.Ensemble(frames)
    before = ens.frames.clone()
    r = ens.cluster("kmedoids", k=1, squared=True)
    assert r.labels.is_cuda and r.n_clusters == 1 and r.iterations == 0 and r.converged
    assert int(r.representatives[0]) == int(ens.medoid()) and int(r.sizes[0]) == 65
    g = ens.cluster(cutoff=0.5, check_every=3)
    assert g.method == "gromos" and g.labels.is_cuda and int(g.sizes.sum()) == 65
    assert torch.equal(ens.frames, before)                           # the ensemble's frames are unchanged
    # NumPy in gives NumPy out
    host = ens.rmsd_matrix().cpu().numpy()
    n = sc.cluster_gromos(host, 0.5)
    assert isinstance(n.labels, np.ndarray) and isinstance(n.representatives, np.ndarray) and isinstance(n.members(0), np.ndarray)
    assert np.array_equal(n.labels, g.labels.cpu().numpy())
    k = sc.cluster_kmedoids(host, 4)
    assert isinstance(k.labels, np.ndarray) and isinstance(k.total_deviation, np.ndarray)
