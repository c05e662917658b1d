"""
NumPy specification of the correlation networks (springcraft_amd/network.py, csrc/corr_network.hip): the edge-weight rule,
plain Floyd-Warshall with a next-hop matrix, and the walk-and-count of a next-hop matrix.  Shared by the host and the GPU
tests; nothing here touches a device.
"""
import numpy as np

INF = np.inf


def edge_weights(corr, coord=None, contact_cutoff=None, min_correlation=0.0):
    """W[a, c] = -log(min(|c_ac|, 1)) on the edges, +inf elsewhere, 0 on the diagonal (a NaN entry is no edge)."""
    c = np.asarray(corr, dtype=np.float64)
    ac = np.abs(c)
    with np.errstate(invalid="ignore"):
        edge = ac >= min_correlation
    if coord is not None:
        x = np.asarray(coord, dtype=np.float64)
        d = x[:, None, :] - x[None, :, :]
        dist_sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        with np.errstate(invalid="ignore"):
            edge &= dist_sq <= np.float64(contact_cutoff) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(edge, np.where(ac >= 1.0, 0.0, -np.log(np.minimum(ac, 1.0))), INF)
    np.fill_diagonal(w, 0.0)
    return w


def input_flag(corr, coord=None):
    """Whether the member has no defined result: a NaN in its map or coordinates."""
    return bool(np.isnan(corr).any() or (coord is not None and np.isnan(coord).any()))


def floyd_warshall(weights):
    """
    (D, S) of non-negative weights: D[i, j] = min(D[i, j], D[i, k] + D[k, j]) for k ascending, updated on strict improvement
    only with S[i, j] <- S[i, k]; S starts as j on a finite edge, i on the diagonal, -1 elsewhere.
    """
    d = np.array(weights, dtype=np.float64)
    n = len(d)
    np.fill_diagonal(d, 0.0)
    s = np.where(d < INF, np.arange(n, dtype=np.int32)[None, :], np.int32(-1)).astype(np.int32)
    s[np.arange(n), np.arange(n)] = np.arange(n)
    for k in range(n):
        cand = d[:, k, None] + d[None, k, :]
        better = cand < d
        d = np.where(better, cand, d)
        s = np.where(better, s[:, k, None], s)
    return d, s


def walk_usage(next_hop):
    """usage[v]: ordered pairs (a, t), a, t, v distinct, t reachable from a, whose walk a -> S[a, t] -> ... -> t passes v."""
    s = np.asarray(next_hop)
    n = len(s)
    usage = np.zeros(n, dtype=np.int64)
    for t in range(n):
        v = s[:, t].astype(np.int64)
        active = (v >= 0) & (v != t)
        active[t] = False
        hops = 0
        while active.any():
            assert hops <= n, "a walk does not end"
            np.add.at(usage, v[active], 1)
            v[active] = s[v[active], t]
            assert (v[active] >= 0).all(), "a walk leaves the graph"
            active &= v != t
            hops += 1
    return usage


def walk(next_hop, a, c):
    """The node list a -> ... -> c of a next-hop matrix, [] if c is not reachable."""
    nodes, v = [a], a
    while v != c:
        v = int(next_hop[v, c])
        if v < 0:
            return []
        nodes.append(v)
        assert len(nodes) <= len(next_hop), "a walk does not end"
    return nodes


def check_paths(weights, dist, next_hop, exact=True):
    """
    For every pair: S == -1 exactly where D is +inf; else the walk is a simple path over finite edges whose weights, added
    in walk order, EQUAL D[a, c].  ``exact=False``, for weights whose sums round and paths of three edges or more: D is
    the same terms added in the order of the pivots, two sums of at most n - 1 non-negative terms, so they differ by at
    most 2 n eps D.  Vectorised over the sources of a target.  Returns the number of walked pairs.
    """
    w = np.array(weights, dtype=np.float64)
    np.fill_diagonal(w, 0.0)
    n = len(w)
    assert np.array_equal(next_hop == -1, dist == INF)
    assert np.array_equal(np.diag(next_hop), np.arange(n)) and not np.diag(dist).any()
    walked = 0
    for t in range(n):
        at = np.arange(n)
        total = np.zeros(n)
        seen = np.zeros((n, n), dtype=bool)
        seen[at, at] = True
        active = (next_hop[:, t] >= 0) & (at != t)
        walked += int(active.sum())
        for _ in range(n):
            if not active.any():
                break
            nxt = next_hop[at[active], t]
            assert (nxt >= 0).all()
            step = w[at[active], nxt]
            assert (step < INF).all(), "the path uses a missing edge"
            assert not seen[np.nonzero(active)[0], nxt].any(), "the path visits a node twice"
            seen[np.nonzero(active)[0], nxt] = True
            total[active] = total[active] + step
            at[active] = nxt
            active &= at != t
        assert not active.any(), "a walk does not end"
        reach = dist[:, t] < INF
        if exact:
            assert np.array_equal(total[reach], dist[reach, t]), f"target {t}: the walk's sum is not D"
        else:
            gate = 2 * n * np.finfo(np.float64).eps * dist[reach, t]
            assert np.all(np.abs(total[reach] - dist[reach, t]) <= gate), f"target {t}: the walk's sum is not D"
    return walked


def dyadic_weights(rng, n, density=1.0, symmetric=True):
    """Weights k / 1024, k in 1..4096 (every path sum is exact in float64) on about ``density`` of the pairs, +inf elsewhere."""
    w = rng.integers(1, 4097, size=(n, n)).astype(np.float64) / 1024.0
    if density < 1.0:
        w[rng.random((n, n)) >= density] = INF
    if symmetric:
        w = np.triu(w, 1)
        w = w + w.T
    np.fill_diagonal(w, 0.0)
    return w
