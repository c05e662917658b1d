"""
CPU-only checks of the clustering: the NumPy specification (tests/cluster_model.py) against independent checks -- planted
groups, closed-form cases, brute-force local optimality on dyadic distances, where every sum is exact -- the argument
validation of springcraft_amd/cluster.py, which happens before a device is touched, the C entries' declarations and
argument checks, and the policy header under sanitizers.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
from os.path import dirname, join

import numpy as np
import pytest

from springcraft_amd import _hip
from tests import cluster_model as cm
from tests import rmsd_matrix_model as rm

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_cluster_workspace": 2, "sc_cluster_form": 2, "sc_dev_cluster_gromos_init_f64": 8,
           "sc_dev_cluster_gromos_rounds": 10, "sc_dev_cluster_kmedoids_init_f64": 12,
           "sc_dev_cluster_kmedoids_swaps_f64": 13}


# ---- the specification: neighbour count ---------------------------------------------------------------------------------------------
def test_gromos_recovers_planted_groups():
    pts, planted = cm.planted_points(np.random.default_rng(1), (40, 25, 25, 9, 1))
    labels, centres, sizes, flag = cm.gromos(cm.euclidean(pts), 1.0)
    assert flag == 0 and sizes.tolist() == [40, 25, 25, 9, 1] and cm.same_partition(labels, planted)
    # every member of a group sees the whole group: the centre is the group's lowest index, and of the two groups of 25
    # the one that holds the lower index comes first
    assert all(c == np.flatnonzero(labels == g)[0] for g, c in enumerate(centres)) and centres[1] < centres[2]


def test_gromos_sizes_do_not_increase():
    d = cm.dyadic_matrix(np.random.default_rng(2), 90)
    for cutoff in (1.0, 2.5, 4.0):
        labels, centres, sizes, _ = cm.gromos(d, cutoff)
        assert np.all(np.diff(sizes) <= 0) and sizes.sum() == 90 and (labels >= 0).all()
        assert np.array_equal(np.bincount(labels), sizes) and len(set(centres.tolist())) == len(centres)


def test_gromos_cutoff_zero_groups_duplicates_only():
    d = cm.dyadic_matrix(np.random.default_rng(3), 20)
    for a, b in ((2, 11), (11, 17), (2, 17), (5, 6)):
        d[a, b] = d[b, a] = 0.0
    labels, centres, sizes, _ = cm.gromos(d, 0.0)
    assert sizes.tolist() == [3, 2] + [1] * 15 and centres[:2].tolist() == [2, 5]
    assert set(np.flatnonzero(labels == 0)) == {2, 11, 17} and set(np.flatnonzero(labels == 1)) == {5, 6}


def test_gromos_huge_cutoff_gives_one_cluster_centred_on_the_first():
    d = cm.dyadic_matrix(np.random.default_rng(4), 33)
    labels, centres, sizes, _ = cm.gromos(d, 100.0)
    assert centres.tolist() == [0] and sizes.tolist() == [33] and not labels.any()
    labels, centres, sizes, _ = cm.gromos(d, 100.0, max_clusters=3)
    assert centres.tolist() == [0]
    labels, centres, sizes, _ = cm.gromos(d, 0.0, max_clusters=3)
    assert centres.tolist() == [0, 1, 2] and labels[:4].tolist() == [0, 1, 2, -1]


def test_gromos_invalid_items_and_the_flag():
    d = cm.dyadic_matrix(np.random.default_rng(5), 12)
    d[4, :] = d[:, 4] = np.nan
    labels, centres, sizes, flag = cm.gromos(d, 3.0)
    keep = np.delete(np.arange(12), 4)
    sub = cm.gromos(d[np.ix_(keep, keep)], 3.0)
    assert flag == 0 and labels[4] == -1 and np.array_equal(labels[keep], sub[0])
    assert np.array_equal(centres, keep[sub[1]]) and np.array_equal(sizes, sub[2])
    d[2, 7] = np.nan
    labels, centres, sizes, flag = cm.gromos(d, 3.0)
    assert flag == 1 and (labels == -1).all() and len(centres) == 0


# ---- the specification: k-medoids ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k", [(30, 2), (30, 5), (45, 3), (45, 8)])
def test_kmedoids_dyadic_strictly_decreasing_to_a_local_optimum(n, k):
    d = cm.dyadic_matrix(np.random.default_rng([n, k]), n)
    r = cm.kmedoids(d, k)
    assert r["converged"] and r["flag"] == 0 and len(r["td"]) == r["iterations"] + 1
    assert np.all(np.diff(r["td"]) < 0)
    med = r["medoids"].tolist()
    valid = np.ones(n, dtype=bool)
    assert r["td"][-1] == cm.total_deviation(d, med, valid)
    # brute force over every (x, s): no exchange lowers the total deviation, and the model's delta is that difference
    delta = cm.swap_deltas(d, med, valid)
    for x in range(n):
        for s in range(k):
            if x in med:
                continue
            trial = list(med)
            trial[s] = x
            change = cm.total_deviation(d, trial, valid) - r["td"][-1]
            assert change >= 0 and change == delta[x, s]
    assert np.array_equal(np.bincount(r["labels"], minlength=k), r["sizes"])


def test_kmedoids_k1_is_the_medoid():
    d = cm.dyadic_matrix(np.random.default_rng(6), 40)
    d[7, :] = d[:, 7] = np.nan
    r = cm.kmedoids(d, 1)
    assert r["medoids"].tolist() == [rm.medoid(d)] and r["iterations"] == 0 and r["converged"]
    assert r["labels"][7] == -1 and r["sizes"].tolist() == [39]
    assert cm.kmedoids(np.array([[0.0, 2.0], [2.0, 0.0]]), 1)["medoids"].tolist() == [0]


def test_kmedoids_recovers_planted_groups_and_k_at_the_item_count():
    pts, planted = cm.planted_points(np.random.default_rng(7), (20, 14, 9, 6))
    r = cm.kmedoids(cm.euclidean(pts), 4)
    assert cm.same_partition(r["labels"], planted) and r["converged"]
    d = cm.dyadic_matrix(np.random.default_rng(8), 6)
    d[3, :] = d[:, 3] = np.nan
    r = cm.kmedoids(d, 6)
    assert sorted(r["medoids"].tolist()) == [0, 1, 2, 4, 5] and r["td"].tolist() == [0.0] and r["iterations"] == 0
    assert r["labels"][3] == -1 and r["sizes"].tolist() == [1] * 5


# ---- host-side argument checks: all raise before any device call (there is no device here) --------------------------------------------
def test_argument_validation_needs_no_device():
    import springcraft_amd as sc
    from springcraft_amd import cluster as cl

    assert sc.cluster_gromos is cl.cluster_gromos and sc.cluster_kmedoids is cl.cluster_kmedoids
    assert sc.Clustering is cl.Clustering and (cl.MAX_ITEMS, cl.MAX_MEDOIDS) == (262144, 1024)
    d = np.zeros((5, 5))
    for bad in (np.zeros((4, 5)), np.zeros(5), np.zeros((2, 3, 3)), np.zeros((0, 0)), np.zeros((5, 5), dtype=np.float32),
                [[0.0, 1.0], [1.0, 0.0]]):
        with pytest.raises(ValueError):
            sc.cluster_gromos(bad, 1.0)
        with pytest.raises(ValueError):
            sc.cluster_kmedoids(bad, 1)
    for cutoff in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="cutoff"):
            sc.cluster_gromos(d, cutoff)
    for kw in (dict(max_clusters=0), dict(check_every=0)):
        with pytest.raises(ValueError):
            sc.cluster_gromos(d, 1.0, **kw)
    for k in (0, 6, -1, None):
        with pytest.raises(ValueError, match="k"):
            sc.cluster_kmedoids(d, k)
    for kw in (dict(max_iter=0), dict(check_every=0)):
        with pytest.raises(ValueError):
            sc.cluster_kmedoids(d, 2, **kw)
    with pytest.raises(ValueError, match="at most"):
        cl.workspace_bytes(262145, 0)
    with pytest.raises(ValueError, match="at most"):
        cl.workspace_bytes(5000, 1025)
    assert cl.check_gromos_args(10, 2, 50, 7) == (2.0, 10, 7) and cl.check_kmedoids_args(10, 10, 1, 1) == (10, 1, 1)


class _Stub:
    """An ensemble's host side alone, for the checks of ``cluster`` that come before any device call."""

    def __init__(self, n_frames):
        from springcraft_amd.ensemble import Ensemble

        self.n_frames = n_frames
        self.cluster = Ensemble.cluster.__get__(self)

    def rmsd_matrix(self, **_):
        raise AssertionError("the matrix was asked for before the arguments were checked")


def test_ensemble_cluster_validation_needs_no_device():
    ens = _Stub(20)
    for kw in (dict(method="ward", cutoff=1.0), dict(method="gromos"), dict(method="kmedoids"), dict(method="gromos", k=3),
               dict(method="kmedoids", cutoff=1.0), dict(method="kmedoids", k=21), dict(method="kmedoids", k=0),
               dict(method="gromos", cutoff=-1.0), dict(method="gromos", cutoff=1.0, max_iter=5),
               dict(method="kmedoids", k=3, max_clusters=5), dict(method="kmedoids", k=3, max_iter=0),
               dict(method="gromos", cutoff=1.0, check_every=0)):
        with pytest.raises(ValueError):
            ens.cluster(**kw)
    with pytest.raises(ValueError, match="at most"):
        _Stub(300000).cluster(method="gromos", cutoff=1.0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entries_declared_exported_and_typed():
    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    assert {n for n in _hip.EXPORTED_SYMBOLS if "cluster" in n} == set(ENTRIES)
    assert all(n.startswith(("sc_cluster_", "sc_dev_cluster_")) for n in ENTRIES)
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\b(?:int|int64_t) {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name


def _closed_form(n, k):
    up = lambda v: (v + 255) // 256 * 256        # noqa: E731
    words = (n + 63) // 64
    regions = [16, 8 * words]
    if k == 0:
        regions += [8 * words, 8 * words, 4 * n, 8 * n * words]
    else:
        regions += [4 * k, 4 * n, 4 * n, 8 * n, 8 * n, 8 * n, 4 * n, 4 * n, 4 * (k + 1), 8 * n, 8 * n, 8 * k, 8 * k]
    off = 0
    for r in regions:
        off = up(off) + r
    return off


@pytest.mark.parametrize("n, k", [(1, 0), (1, 1), (63, 0), (64, 0), (65, 0), (130, 7), (200, 200), (10000, 0), (10000, 100),
                                  (262144, 0), (262144, 1024)])
def test_workspace_closed_form(n, k):
    assert _hip.lib().sc_cluster_workspace(n, k) == _closed_form(n, k)


def test_workspace_refuses_what_cannot_be_indexed():
    ws = _hip.lib().sc_cluster_workspace
    for bad in ((0, 0), (-1, 0), (5, -1), (262145, 0), (2 ** 40, 3), (5, 6), (5000, 1025)):
        assert ws(*bad) == -1, bad
    assert ws(5, 5) > 0 and ws(262144, 1024) > 0


def test_form_policy(monkeypatch):
    form = _hip.lib().sc_cluster_form
    monkeypatch.delenv("SPRINGCRAFT_CLUSTER_FORM", raising=False)
    assert [form(2000, 100), form(8062, 1), form(8063, 1), form(10000, 10)] == [0, 0, 1, 1]
    monkeypatch.setenv("SPRINGCRAFT_CLUSTER_FORM", "stream")
    assert [form(2000, 100), form(10000, 10)] == [1, 1]
    monkeypatch.setenv("SPRINGCRAFT_CLUSTER_FORM", "lds")        # never beyond what fits
    assert [form(2000, 100), form(10000, 10)] == [0, 1]


def test_entries_refuse_a_missing_context():
    """A NULL context answers SC_ERR_INVALID_ARG before anything else (the range checks need a context: test_cluster_gpu.py)."""
    L = _hip.lib()
    bad = _hip.SC_ERR_INVALID_ARG
    p = C.c_void_p(256)        # (never dereferenced)
    assert L.sc_dev_cluster_gromos_init_f64(None, p, 5, 1.0, p, 1 << 20, p, p) == bad
    assert L.sc_dev_cluster_gromos_rounds(None, 5, 1, 5, p, 1 << 20, p, p, p, p) == bad
    assert L.sc_dev_cluster_kmedoids_init_f64(None, p, 5, 2, p, 1 << 20, p, p, p, p, 4, p) == bad
    assert L.sc_dev_cluster_kmedoids_swaps_f64(None, p, 5, 2, 1, p, 1 << 20, p, p, p, p, 4, p) == bad


# ---- the policy header under sanitizers -------------------------------------------------------------------------------------------
def test_cluster_policy_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_cluster_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_cluster_policy.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "SPRINGCRAFT_CLUSTER_FORM"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "cluster policy ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
