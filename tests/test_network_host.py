"""
CPU-only checks of the correlation networks: the NumPy specification (tests/network_model.py) against SciPy's
Floyd-Warshall and, on graphs without ties, networkx's betweenness; the host arithmetic of springcraft_amd/network.py and
its argument validation, which happens before a device is touched.
"""
import numpy as np
import pytest

from tests import network_model as nm


@pytest.mark.parametrize("n, density, symmetric", [(1, 1.0, True), (2, 1.0, True), (40, 1.0, True), (65, 0.05, True),
                                                   (130, 0.05, False), (50, 1.0, False)])
def test_specification_matches_scipy(n, density, symmetric):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    w = nm.dyadic_weights(np.random.default_rng(n), n, density, symmetric)
    d, s = nm.floyd_warshall(w)
    ref = csgraph.floyd_warshall(np.where(np.isinf(w), 0.0, w), directed=True)   # (a dense 0 is "no edge" to SciPy)
    assert np.array_equal(d, ref)                                             # dyadic weights: every sum is exact
    assert nm.check_paths(w, d, s) == int(np.isfinite(d).sum()) - n
    if symmetric:
        assert np.array_equal(d, d.T)


def test_specification_generic_weights_within_the_gate():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(5)
    n = 90
    w = rng.uniform(0.5, 2.0, size=(n, n))
    w = np.triu(w, 1) + np.triu(w, 1).T
    d, _ = nm.floyd_warshall(w)
    ref = csgraph.floyd_warshall(w, directed=False)
    assert np.all(np.abs(d - ref) <= 2 * n * np.finfo(np.float64).eps * ref)
    assert np.array_equal(d, d.T)


def _random_tree(rng, n):
    w = np.full((n, n), 1000.0)
    edges = []
    for v in range(1, n):
        u = int(rng.integers(0, v))
        w[u, v] = w[v, u] = float(rng.integers(1, 4097)) / 1024.0
        edges.append((u, v))
    np.fill_diagonal(w, 0.0)
    return w, edges


def test_usage_matches_networkx_on_a_tree():
    nx = pytest.importorskip("networkx")
    n = 60
    w, _ = _random_tree(np.random.default_rng(3), n)
    _, s = nm.floyd_warshall(w)
    g = nx.from_numpy_array(w)
    bc = nx.betweenness_centrality(g, weight="weight", normalized=False, endpoints=False)
    assert np.array_equal(nm.walk_usage(s), np.array([2 * bc[v] for v in range(n)]).astype(np.int64))


def test_usage_closed_forms():
    n = 17
    path = np.full((n, n), np.inf)
    star = np.full((n, n), np.inf)
    for i in range(n - 1):
        path[i, i + 1] = path[i + 1, i] = 1.0
        star[0, i + 1] = star[i + 1, 0] = 1.0
    i = np.arange(n)
    assert np.array_equal(nm.walk_usage(nm.floyd_warshall(path)[1]), 2 * i * (n - 1 - i))
    want = np.zeros(n, dtype=np.int64)
    want[0] = (n - 1) * (n - 2)
    assert np.array_equal(nm.walk_usage(nm.floyd_warshall(star)[1]), want)


def test_weight_rule():
    c = np.array([[1.0, -0.5, 0.05, 1.0000001], [-0.5, 1.0, 0.0, 0.3], [0.05, 0.0, 1.0, -1.5], [1.0000001, 0.3, -1.5, 1.0]])
    w = nm.edge_weights(c, min_correlation=0.1)
    assert w[0, 1] == -np.log(0.5) and np.isinf(w[0, 2]) and np.isinf(w[1, 2])
    assert w[0, 3] == 0.0 and w[2, 3] == 0.0 and not np.diag(w).any()
    assert nm.edge_weights(c)[1, 2] == np.inf and nm.edge_weights(c)[0, 2] == -np.log(0.05)
    x = np.array([[0.0, 0, 0], [3.0, 0, 0], [0, 4.0, 0], [3.0, 4.0, 0]])
    w = nm.edge_weights(c, x, 4.0, 0.0)
    assert np.isfinite(w[0, 1]) and np.isfinite(w[0, 2]) and np.isinf(w[0, 3]) and np.isinf(w[1, 2])   # 3, 4, 5, 5
    c[1, 2] = np.nan
    assert nm.input_flag(c) and np.isinf(nm.edge_weights(c)[1, 2])


def test_member_records_and_forms():
    from springcraft_amd import network as net

    rec = net.member_records([5, 64, 129])
    assert rec.dtype == np.int64 and rec.tolist() == [[5, 0, 0], [64, 25, 5], [129, 25 + 4096, 69]]
    assert net.member_records([7] * 3)[:, 1].tolist() == [0, 49, 98]
    with pytest.raises(ValueError):
        net.check_sizes([])
    with pytest.raises(ValueError):
        net.check_sizes([4, 0])
    with pytest.raises(ValueError):
        net.check_sizes([1] * 65536)
    with pytest.raises(ValueError):
        net.check_sizes([262145])


def test_argument_validation_needs_no_device():
    import springcraft_amd as sc
    from springcraft_amd import network as net

    c = np.eye(4)
    x = np.zeros((4, 3))
    for kw in [dict(min_correlation=-0.1), dict(min_correlation=1.5), dict(min_correlation=float("nan")),
               dict(contact_cutoff=8.0), dict(coord=x), dict(coord=x, contact_cutoff=0.0),
               dict(coord=x, contact_cutoff=-1.0), dict(coord=x, contact_cutoff=float("inf"))]:
        with pytest.raises(ValueError):
            sc.correlation_network(c, **kw)
    for bad in [np.zeros((3, 4)), np.zeros((2, 3, 4)), np.zeros(5), [], [np.zeros((2, 2)), np.zeros((2, 3))]]:
        with pytest.raises(ValueError):
            sc.shortest_paths(bad)
        with pytest.raises(ValueError):
            sc.correlation_network(bad)
    assert net.check_network_args(0.25, None, False) == (0.25, None)
    assert net.check_network_args(1, 7, True) == (1.0, 7.0)
    assert sc.CorrelationNetwork is net.CorrelationNetwork and net.USAGE_MAX_NODES == 8192


def test_model_validation_needs_no_device():
    import springcraft_amd as sc

    coord = np.random.default_rng(0).random((10, 3)) * 10
    anm = sc.ANM(coord, sc.InvariantForceField(7.0))
    gnm = sc.GNM(coord, sc.InvariantForceField(7.0))
    with pytest.raises(ValueError):
        anm.correlation_network(min_correlation=2.0)
    with pytest.raises(ValueError):
        anm.correlation_network(contact_cutoff=0.0)
    with pytest.raises(ValueError):
        anm.correlation_network(kind="prs")
    with pytest.raises(ValueError):
        sc.nma.correlation_network(gnm, kind="lmi")
