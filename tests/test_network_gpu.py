"""
GPU checks of the correlation networks (csrc/corr_network.hip, springcraft_amd/network.py) against the NumPy specification
of tests/network_model.py.

Exact cases have dyadic weights k / 1024, k in 1..4096: every path sum is exact in float64, so the distances must EQUAL the
specification's whatever the order of the pivots.  Generic cases have weights in [0.5, 2]: each side sums at most n - 1
non-negative terms, each sum with a relative error of at most (n - 2) eps to first order, so the two minima differ by at
most 2 n eps D.  The next hops may differ from the specification's on ties; they are checked by what they promise: the walk
is a simple path over finite edges whose weights, added in walk order, equal D.
"""
import ctypes as C

import numpy as np
import pytest

from tests import network_model as nm
from tests.util import structures

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 63, 64, 65, 130, 200]
RAGGED = (5, 64, 129)


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


_cases = {}


def exact_case(n, density, symmetric=True, members=3):
    """(weights (members, n, n), [(D, S) of the specification]) with dyadic weights, computed once."""
    key = (n, density, symmetric, members)
    if key not in _cases:
        rng = np.random.default_rng([n, int(100 * density), int(symmetric), members])
        w = np.stack([nm.dyadic_weights(rng, n, density, symmetric) for _ in range(members)])
        if density < 1.0 and n > 2:
            # a sparse graph of 130 nodes or more is connected all the same: the last tenth of the nodes is a part of its own
            k = n - max(1, n // 10)
            w[:, :k, k:] = w[:, k:, :k] = np.inf
        ref = [nm.floyd_warshall(m) for m in w]
        for a in (w, *[x for r in ref for x in r]):
            a.setflags(write=False)
        _cases[key] = (w, ref)
    return _cases[key]


# ---- exact distances, paths and usage ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [1.0, 0.05])
@pytest.mark.parametrize("n", SIZES)
def test_exact_batch_of_three(sc, n, density):
    w, ref = exact_case(n, density)
    net = sc.network.network_of_weights(w)
    d, s = net.distances, net.next_hop
    assert isinstance(d, np.ndarray) and d.shape == (3, n, n) and d.dtype == np.float64 and s.dtype == np.int32
    usage = net.usage
    assert usage.shape == (3, n) and usage.dtype == np.int64 and not net.flags.any()
    for b in range(3):
        assert np.array_equal(d[b], ref[b][0]), f"member {b}"
        assert np.array_equal(d[b], d[b].T)
        nm.check_paths(w[b], d[b], s[b])
        assert np.array_equal(usage[b], nm.walk_usage(s[b]))
    if density < 1.0 and n >= 63:
        assert np.isinf(d).any() and np.isfinite(d).sum() > 3 * n      # unreachable pairs and real paths
    # a member's bits do not depend on the batch, its position or its neighbours
    d1, s1 = sc.shortest_paths(w[1])
    assert d1.shape == (n, n) and np.array_equal(d1, d[1]) and np.array_equal(s1, s[1])
    d2, s2 = sc.shortest_paths(np.stack([w[2], w[1]]))
    assert np.array_equal(d2[1], d[1]) and np.array_equal(s2[1], s[1]) and np.array_equal(d2[0], d[2])


def test_exact_directed_network(sc):
    w, ref = exact_case(130, 0.05, symmetric=False, members=1)
    net = sc.network.network_of_weights(w[0])
    assert np.array_equal(net.distances, ref[0][0]) and not np.array_equal(net.distances, net.distances.T)
    nm.check_paths(w[0], net.distances, net.next_hop)
    assert np.array_equal(net.usage, nm.walk_usage(net.next_hop))


def test_ragged_members_have_the_bits_of_their_uniform_solve(sc, torch):
    rng = np.random.default_rng(11)
    maps = [nm.dyadic_weights(rng, n, 1.0 if n < 100 else 0.05) for n in RAGGED]
    net = sc.network.network_of_weights(maps)
    assert isinstance(net.distances, list) and [m.shape for m in net.distances] == [(n, n) for n in RAGGED]
    for b, w in enumerate(maps):
        d, s = sc.shortest_paths(w)
        assert np.array_equal(net.distances[b], nm.floyd_warshall(w)[0])
        assert np.array_equal(net.distances[b], d) and np.array_equal(net.next_hop[b], s)
        nm.check_paths(w, d, s)
        assert np.array_equal(net.usage[b], nm.walk_usage(s))
    # the same from device tensors: views of packed buffers come back, nothing is copied to the host
    dev = sc.network.network_of_weights([torch.from_numpy(w).cuda() for w in maps[::-1]])
    assert dev.distances[0].is_cuda and dev.next_hop[0].dtype == torch.int32
    assert dev.distances[0].untyped_storage().data_ptr() == dev.distances[2].untyped_storage().data_ptr()
    for b in range(3):
        assert np.array_equal(dev.distances[b].cpu().numpy(), net.distances[2 - b])
        assert np.array_equal(dev.next_hop[b].cpu().numpy(), net.next_hop[2 - b])
        assert np.array_equal(dev.usage[b].cpu().numpy(), net.usage[2 - b])


# ---- generic weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [65, 200])
def test_generic_weights_within_the_gate(sc, n, symmetric):
    rng = np.random.default_rng(n + symmetric)
    w = rng.uniform(0.5, 2.0, size=(2, n, n))
    if symmetric:
        w = np.triu(w, 1) + np.triu(w, 1).transpose(0, 2, 1)
    w[:, np.arange(n), np.arange(n)] = 0.0
    d, s = sc.shortest_paths(w)
    for b in range(2):
        ref = nm.floyd_warshall(w[b])[0]
        err = np.abs(d[b] - ref)
        gate = 2 * n * EPS * ref
        print(f"n={n} symmetric={symmetric} member {b}: max error / gate = {np.max(err[ref > 0] / gate[ref > 0]):.3f}")
        assert np.all(err <= gate)
        assert (s[b] >= 0).all()
        if symmetric:
            assert np.array_equal(d[b], d[b].T)


# ---- usage: closed forms and networkx -------------------------------------------------------------------------------------------------
def test_usage_closed_forms(sc):
    n = 130
    path = np.full((n, n), np.inf)
    star = np.full((n, n), np.inf)
    for i in range(n - 1):
        path[i, i + 1] = path[i + 1, i] = 1.0
        star[0, i + 1] = star[i + 1, 0] = 1.0
    net = sc.network.network_of_weights(np.stack([path, star]))
    i = np.arange(n)
    hub = np.zeros(n, dtype=np.int64)
    hub[0] = (n - 1) * (n - 2)
    assert np.array_equal(net.usage[0], 2 * i * (n - 1 - i)) and np.array_equal(net.usage[1], hub)
    assert net.betweenness()[1][0] == 1.0 and np.array_equal(net.betweenness(normalized=False), net.usage.astype(np.float64))
    assert np.array_equal(net.distances[0], np.abs(i[:, None] - i[None, :]).astype(np.float64))
    assert net.path(3, 7) == [3, 4, 5, 6, 7] and net.path(9, 9) == [9] and net.path(5, 99, member=1) == [5, 0, 99]
    assert net.path_length(3, 7) == 4.0 and net.path_length(5, 99, member=1) == 2.0 and net.reachable().all()
    with pytest.raises(IndexError):
        net.path(0, n)
    with pytest.raises(IndexError):
        net.path(0, 1, member=2)
    # two components: no path between them, in either direction
    two = path.copy()
    two[64, 65] = two[65, 64] = np.inf
    cut = sc.network.network_of_weights(two)
    assert cut.path(0, 129) == [] and cut.path_length(129, 0) == np.inf
    assert np.array_equal(cut.reachable(), (i[:, None] < 65) == (i[None, :] < 65))
    assert np.array_equal(cut.next_hop == -1, ~cut.reachable())
    left, right = np.arange(65), np.arange(65)
    assert np.array_equal(cut.usage, np.concatenate([2 * left * (64 - left), 2 * right * (64 - right)]))


def test_usage_matches_networkx_on_a_tree(sc):
    nx = pytest.importorskip("networkx")
    n = 130
    rng = np.random.default_rng(3)
    w = np.full((n, n), 1000.0)          # no shortest path takes a filler edge: a tree path is at most 129 * 4 long
    for v in range(1, n):
        u = int(rng.integers(0, v))
        w[u, v] = w[v, u] = float(rng.integers(1, 4097)) / 1024.0
    np.fill_diagonal(w, 0.0)
    net = sc.network.network_of_weights(w)
    bc = nx.betweenness_centrality(nx.from_numpy_array(w), weight="weight", normalized=False, endpoints=False)
    want = np.array([2 * bc[v] for v in range(n)])
    assert np.array_equal(net.usage, want.astype(np.int64))
    assert np.array_equal(net.betweenness(), want / ((n - 1) * (n - 2)))


def test_usage_beyond_the_lds_limit_is_refused_before_a_launch(sc, torch):
    from springcraft_amd import _hip

    ctx, L = _hip.context(), _hip.lib()
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert L.sc_dev_net_usage(ctx.handle, p, 1, 8192 + 1, 4, p, p, p) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_net_usage(ctx.handle, p, 0, 4, 4, p, p, p) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_net_paths_f64(ctx.handle, p, 65536, 4, p, p, p, p) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_net_weights_f64(ctx.handle, p, 1, 2, p, None, 0.0, 1.5, p, p) == _hip.SC_ERR_INVALID_ARG
    assert L.sc_dev_net_workspace(0) == -1 and L.sc_dev_net_workspace(5) == 20 and L.sc_dev_net_workspace(4096) == 16384


# ---- the weight kernel ---------------------------------------------------------------------------------------------------------------
def weight_inputs(n=130, members=2):
    rng = np.random.default_rng(17)
    c = rng.uniform(-1.0, 1.0, size=(members, n, n))
    c = (c + c.transpose(0, 2, 1)) / 2
    c[:, 3, 5] = c[:, 5, 3] = 1.0 + 2.0 ** -40          # slightly above 1: weight 0
    c[:, 7, 9] = c[:, 9, 7] = -1.25
    c[:, 2, 4] = c[:, 4, 2] = 0.0                        # -log 0: no edge
    c[:, np.arange(n), np.arange(n)] = 1.0
    x = rng.uniform(0.0, 30.0, size=(members, n, 3))
    x[:, 0] = np.array([1.0, 2.0, 3.0])
    x[:, 1] = np.array([4.0, 6.0, 3.0])                 # at the cutoff 5 exactly: in contact
    return c, x


@pytest.mark.parametrize("min_correlation, cutoff", [(0.0, None), (0.3, None), (0.0, 5.0), (0.3, 12.0), (1.0, None)])
def test_weight_kernel_against_the_specification(sc, min_correlation, cutoff):
    c, x = weight_inputs()
    net = sc.correlation_network(c, None if cutoff is None else x, cutoff, min_correlation)
    assert not net.flags.any()
    for b in range(len(c)):
        ref = nm.edge_weights(c[b], None if cutoff is None else x[b], cutoff, min_correlation)
        got = net.weights[b]
        finite = np.isfinite(ref)
        assert np.array_equal(np.isinf(got), ~finite) and not np.diag(got).any() and not np.signbit(got[finite]).any()
        ulp = np.abs(got[finite] - ref[finite]) / np.spacing(np.maximum(ref[finite], np.finfo(np.float64).tiny))
        print(f"min_correlation={min_correlation} cutoff={cutoff} member {b}: edges {int(finite.sum())}, max {ulp.max():.2f} ulp")
        assert ulp.max() <= 4
        assert got[3, 5] == 0.0 and got[7, 9] == 0.0 or cutoff is not None
        # the paths are the specification's on the device's own weights, within the generic gate
        d_ref = nm.floyd_warshall(got)[0]
        reach = np.isfinite(d_ref)
        assert np.array_equal(np.isfinite(net.distances[b]), reach)
        assert np.all(np.abs(net.distances[b][reach] - d_ref[reach]) <= 2 * len(got) * EPS * d_ref[reach])
        assert np.array_equal(net.distances[b], net.distances[b].T)
    if cutoff == 5.0:
        assert np.isfinite(net.weights[0][0, 1])


def test_a_nan_member_is_nan_and_the_others_are_untouched(sc):
    c, x = weight_inputs(n=70, members=3)
    clean = sc.correlation_network(c, x, 12.0, 0.1)
    bad_c, bad_x = c.copy(), x.copy()
    bad_c[1, 69, 2] = np.nan                              # one entry, in the last partial tile
    bad_x[2, 5, 1] = np.nan
    net = sc.correlation_network(bad_c, bad_x, 12.0, 0.1)
    assert net.flags.tolist() == [0, 1, 1] and clean.flags.tolist() == [0, 0, 0]
    assert np.isnan(net.distances[1:]).all() and (net.next_hop[1:] == -1).all()
    assert np.array_equal(net.distances[0], clean.distances[0]) and np.array_equal(net.next_hop[0], clean.next_hop[0])
    assert np.array_equal(net.usage[0], clean.usage[0]) and (net.usage[1:] == -1).all()
    assert np.isnan(net.betweenness()[1:]).all() and not net.reachable()[1:].any() and net.path(0, 1, member=1) == []
    # weights handed in directly: a NaN and a negative one
    w = nm.dyadic_weights(np.random.default_rng(2), 70) * np.ones((3, 1, 1))
    w[0, 4, 66] = np.nan
    w[2, 65, 1] = -0.5
    d, s = sc.shortest_paths(w)
    assert np.isnan(d[0]).all() and np.isnan(d[2]).all() and (s[0] == -1).all() and (s[2] == -1).all()
    assert np.array_equal(d[1], nm.floyd_warshall(w[1])[0])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def check_against_the_map(net_w, net_d, net_s, corr, what):
    """
    The device's network of one member against the specification applied to the map ``corr``.  The weights are -log within
    4 ulp, so every path sum of the device's weights is within 4 eps of the specification's, relative, on top of the
    summation's 2 n eps: the gate of the distances.  The path-sum identity is exact, on the device's own weights: the maps
    of these 20-atom models are dense and their stored paths have at most two edges, one addition.
    """
    n = len(corr)
    w_ref = nm.edge_weights(corr)
    finite = np.isfinite(w_ref)
    assert np.array_equal(np.isfinite(net_w), finite)
    assert np.all(np.abs(net_w[finite] - w_ref[finite]) <= 4 * np.spacing(np.maximum(w_ref[finite], np.finfo(np.float64).tiny)))
    d_ref = nm.floyd_warshall(w_ref)[0]
    err = np.abs(net_d - d_ref)
    gate = (2 * n + 4) * EPS * d_ref
    print(f"{what}: max error / gate = {np.max(err[d_ref > 0] / gate[d_ref > 0]):.3f}")
    assert np.all(err <= gate)
    walked = nm.check_paths(net_w, net_d, net_s)
    assert walked == n * (n - 1)


def test_end_to_end_uniform_batch(sc, torch):
    from springcraft_amd.batch import DeviceBatchSolver

    x = structures()["1l2y_coord"].astype(np.float64)
    coords = np.stack([x, x[::-1].copy()])
    s = DeviceBatchSolver(20, 2, sc.InvariantForceField(13.0))
    s.solve(torch.from_numpy(coords).cuda())
    s.finish()
    net = s.correlation_network("dcc")
    assert net.distances.is_cuda and tuple(net.distances.shape) == (2, 20, 20) and net.next_hop.dtype == torch.int32
    corr = s.dcc().cpu().numpy()
    for b in range(2):
        check_against_the_map(net.weights[b].cpu().numpy(), net.distances[b].cpu().numpy(), net.next_hop[b].cpu().numpy(),
                              corr[b], f"uniform dcc member {b}")
    assert np.array_equal(net.usage.cpu().numpy()[0], nm.walk_usage(net.next_hop[0].cpu().numpy()))
    assert not net.flags.any()
    # a contact network on the solver's coordinates and a threshold
    xyz = torch.from_numpy(coords).cuda()
    cut = s.correlation_network("dcc", coord=xyz, contact_cutoff=8.0, min_correlation=0.05)
    for b in range(2):
        w_ref = nm.edge_weights(corr[b], coords[b], 8.0, 0.05)
        assert np.array_equal(np.isfinite(cut.weights[b].cpu().numpy()), np.isfinite(w_ref))
        # (a contact network has paths of many edges: their sums round, in the order of the pivots)
        nm.check_paths(cut.weights[b].cpu().numpy(), cut.distances[b].cpu().numpy(), cut.next_hop[b].cpu().numpy(), exact=False)
    lmi = s.correlation_network("lmi")
    check_against_the_map(lmi.weights[1].cpu().numpy(), lmi.distances[1].cpu().numpy(), lmi.next_hop[1].cpu().numpy(),
                          s.generalized_correlation()[1].cpu().numpy(), "uniform lmi member 1")
    for kw in [dict(min_correlation=1.5), dict(contact_cutoff=8.0), dict(coord=xyz), dict(kind="prs"),
               dict(coord=xyz, contact_cutoff=-1.0)]:
        with pytest.raises(ValueError):
            s.correlation_network(**kw)
    gnm = DeviceBatchSolver(20, 1, sc.InvariantForceField(13.0), dim=1)
    with pytest.raises(ValueError, match=r"abs\(dcc\(norm=True\)\)"):
        gnm.correlation_network("lmi")
    gnm.solve(torch.from_numpy(x[None]).cuda())
    gnm.finish()
    g = gnm.correlation_network()
    check_against_the_map(g.weights[0].cpu().numpy(), g.distances[0].cpu().numpy(), g.next_hop[0].cpu().numpy(),
                          gnm.dcc()[0].cpu().numpy(), "uniform gnm dcc")


def test_end_to_end_ragged_batch(sc, torch):
    from springcraft_amd.batch import RaggedBatchSolver

    x = structures()["1l2y_coord"].astype(np.float64)
    sizes = (20, 15)
    s = RaggedBatchSolver(sizes, sc.InvariantForceField(13.0))
    s.solve(torch.from_numpy(np.concatenate([x, x[:15]])).cuda())
    s.finish()
    net = s.correlation_network("dcc")
    corr = s.dcc()
    assert isinstance(net.distances, list) and [tuple(d.shape) for d in net.distances] == [(20, 20), (15, 15)]
    for b in range(2):
        check_against_the_map(net.weights[b].cpu().numpy(), net.distances[b].cpu().numpy(), net.next_hop[b].cpu().numpy(),
                              corr[b].cpu().numpy(), f"ragged dcc member {b}")
        # the member's bits are those of a network of its own map
        alone = sc.correlation_network(corr[b])
        assert torch.equal(alone.distances, net.distances[b]) and torch.equal(alone.next_hop, net.next_hop[b])
        assert np.array_equal(net.usage[b].cpu().numpy(), nm.walk_usage(net.next_hop[b].cpu().numpy()))


def test_end_to_end_single_model(sc):
    x = structures()["1l2y_coord"].astype(np.float64)
    anm = sc.ANM(x, sc.InvariantForceField(13.0))
    net = anm.correlation_network("lmi")
    assert isinstance(net.distances, np.ndarray) and net.distances.shape == (20, 20)
    check_against_the_map(net.weights, net.distances, net.next_hop, anm.generalized_correlation(), "ANM lmi")
    assert np.array_equal(net.usage, nm.walk_usage(net.next_hop))
    dcc = anm.correlation_network("dcc", contact_cutoff=8.0)
    assert np.array_equal(np.isfinite(dcc.weights), np.isfinite(nm.edge_weights(anm.dcc(), x, 8.0)))
    gnm = sc.GNM(x, sc.InvariantForceField(13.0))
    with pytest.raises(ValueError):
        sc.nma.correlation_network(gnm, kind="lmi")
    g = gnm.correlation_network()
    check_against_the_map(g.weights, g.distances, g.next_hop, gnm.dcc(), "GNM dcc")
