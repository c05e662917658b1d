"""
What tests/test_cluster_host.py and tests/test_cluster_gpu.py share: the NumPy specification of the two clustering methods
of springcraft_amd/cluster.py, plain loops over rounds, and the builders of their inputs.

Common rules.  ``dist`` is (M, M) float64; row i is what item i sees.  Item i is invalid when ``dist[i, i]`` is NaN: label
-1, it neither counts nor is counted, never a representative.  A NaN between two valid items: ``flag`` = 1, every label -1,
no clusters.  Ties go to the lowest index.

Neighbour count (Daura et al. 1999).  ``near[i, j] = dist[i, j] <= cutoff or i == j`` over valid i, j (an item is its own
neighbour whatever its diagonal says, so every round removes its centre).  Until nothing is alive or ``max_clusters``
clusters exist: the alive item with the most alive neighbours, the lowest index among equals, is the centre; its alive
neighbours get the next label and leave.  Comparisons only: a pure function of the matrix' bits.

k-medoids (PAM).  The distance of item j to the medoid in slot s is ``dist[medoid[s], j]``, the medoid's row.  ``dn`` / ``ds``:
an item's distances to its nearest and second-nearest medoid, slots ascending, strict improvement only.  BUILD: the valid
item with the smallest row sum over valid j, then the valid non-medoid with the largest ``sum_j max(dn[j] - dist[i, j], 0)``,
until k medoids or no candidate.  SWAP: ``delta(x, s) = loss[s] + sum_j term`` with ``loss[s] = sum_{nearest(j) = s} (ds[j] -
dn[j])`` and, for ``d = dist[x, j]``: ``d < dn[j]`` adds ``d - dn[j]`` to every slot and ``dn[j] - ds[j]`` to j's own;
else ``d < ds[j]`` adds ``d - ds[j]`` to j's own.  The smallest delta, lowest x then lowest s; below 0: swap and go on.
Sums are float64 (``dtype=np.longdouble`` evaluates delta in extended precision).
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def validity(dist):
    """(valid (M,) bool, flag): the items with a diagonal that is not NaN; whether a NaN lies between two valid items."""
    valid = ~np.isnan(np.diag(dist))
    return valid, int(np.isnan(dist[np.ix_(valid, valid)]).any())


# ---- neighbour count ------------------------------------------------------------------------------------------------------------
def gromos(dist, cutoff, max_clusters=None):
    """``(labels (M,) int32, centres, sizes, flag)``."""
    dist = np.asarray(dist, dtype=np.float64)
    n = len(dist)
    labels = np.full(n, -1, dtype=np.int32)
    valid, flag = validity(dist)
    if flag:
        return labels, np.zeros(0, np.int32), np.zeros(0, np.int32), 1
    with np.errstate(invalid="ignore"):
        near = (dist <= cutoff) | np.eye(n, dtype=bool)
    near &= valid[:, None] & valid[None, :]
    alive = valid.copy()
    centres, sizes = [], []
    while alive.any() and (max_clusters is None or len(centres) < max_clusters):
        count = (near & alive[None, :]).sum(axis=1)
        count[~alive] = -1
        centre = int(np.argmax(count))            # (the first of the largest)
        members = near[centre] & alive
        labels[members] = len(centres)
        alive &= ~members
        centres.append(centre)
        sizes.append(int(members.sum()))
    return labels, np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32), 0


# ---- k-medoids ---------------------------------------------------------------------------------------------------------------------
def assign(dist, medoids, valid):
    """``(nearest (M,) int, dn, ds)`` of the valid items along the medoids' rows (-1 / inf for an invalid item)."""
    n = len(dist)
    nearest = np.full(n, -1)
    dn, ds = np.full(n, np.inf), np.full(n, np.inf)
    for s, m in enumerate(medoids):          # (every item j at once: nearer than dn, else nearer than ds)
        with np.errstate(invalid="ignore"):
            d = dist[m]
            nearer = valid & ((nearest < 0) | (d < dn))
            second = valid & ~nearer & (d < ds)
        ds = np.where(nearer, dn, np.where(second, d, ds))
        dn = np.where(nearer, d, dn)
        nearest = np.where(nearer, s, nearest)
    return nearest, dn, ds


def swap_deltas(dist, medoids, valid, dtype=np.float64):
    """(M, k) delta(x, s) in the arithmetic of ``dtype``; +inf for an x that is invalid or a medoid."""
    n, k = len(dist), len(medoids)
    nearest, dn, ds = assign(dist, medoids, valid)
    items = np.flatnonzero(valid)
    dn_t, ds_t = dn.astype(dtype), ds.astype(dtype)
    loss = np.zeros(k, dtype=dtype)
    for j in items:
        loss[nearest[j]] += ds_t[j] - dn_t[j]
    out = np.full((n, k), np.inf, dtype=dtype)
    for x in items:
        if x in medoids:
            continue
        own = np.zeros(k, dtype=dtype)
        shared = dtype(0)
        for j in items:
            d = dtype(dist[x, j])
            if d < dn_t[j]:
                shared += d - dn_t[j]
                own[nearest[j]] += dn_t[j] - ds_t[j]
            elif d < ds_t[j]:
                own[nearest[j]] += d - ds_t[j]
        out[x] = loss + own + shared
    return out


def kmedoids(dist, k, max_iter=100):
    """
    ``dict``: labels (M,) int32, medoids, sizes, td (the total deviation after BUILD and after every accepted swap),
    iterations, converged, flag.
    """
    dist = np.asarray(dist, dtype=np.float64)
    n = len(dist)
    valid, flag = validity(dist)
    if flag:
        return dict(labels=np.full(n, -1, np.int32), medoids=np.zeros(0, np.int32), sizes=np.zeros(0, np.int32),
                    td=np.zeros(0), iterations=0, converged=True, flag=1)
    items = np.flatnonzero(valid)
    medoids = []
    dn = np.full(n, np.inf)
    while len(medoids) < k:
        best, best_gain = -1, 0.0
        for i in items:
            if i in medoids:
                continue
            row = dist[i, items]
            gain = -row.sum() if not medoids else np.maximum(dn[items] - row, 0.0).sum()
            if best < 0 or gain > best_gain:
                best, best_gain = int(i), gain
        if best < 0:
            break
        medoids.append(best)
        dn = assign(dist, medoids, valid)[1]
    td = [dn[items].sum()]
    iterations, converged = 0, len(medoids) < 2
    for _ in range(max_iter if not converged else 0):
        delta = swap_deltas(dist, medoids, valid)
        x, s = np.unravel_index(np.argmin(delta), delta.shape) if delta.size else (0, 0)   # (the first of the smallest)
        if not delta.size or not delta[x, s] < 0:
            converged = True
            break
        medoids[s] = int(x)
        iterations += 1
        td.append(assign(dist, medoids, valid)[1][items].sum())
    nearest = assign(dist, medoids, valid)[0]
    return dict(labels=nearest.astype(np.int32), medoids=np.array(medoids, dtype=np.int32),
                sizes=np.bincount(nearest[nearest >= 0], minlength=len(medoids)).astype(np.int32), td=np.array(td),
                iterations=iterations, converged=converged, flag=0)


def total_deviation(dist, medoids, valid=None):
    valid = validity(dist)[0] if valid is None else valid
    return assign(dist, list(medoids), valid)[1][valid].sum()


def same_partition(labels_a, labels_b):
    """Whether two labelings group the items alike (the numbering may differ)."""
    pairs = set(zip(np.asarray(labels_a).tolist(), np.asarray(labels_b).tolist()))
    return len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def dyadic_matrix(rng, n):
    """Symmetric, zero diagonal, off-diagonal entries multiples of 2^-10 in (0, 8): every sum of them is exact in float64."""
    a = rng.integers(1, 8192, size=(n, n)).astype(np.float64) / 1024.0
    a = np.triu(a, 1)
    return a + a.T


def planted_points(rng, sizes, spread=0.05, separation=10.0, dim=3):
    """(points, planted labels): groups of the given sizes around centres ``separation`` apart, shuffled."""
    pts, lab = [], []
    for g, m in enumerate(sizes):
        centre = np.zeros(dim)
        centre[g % dim] = separation * (1 + g // dim)
        pts.append(centre + spread * rng.standard_normal((m, dim)))
        lab += [g] * m
    order = rng.permutation(len(lab))
    return np.concatenate(pts)[order], np.array(lab)[order]


def euclidean(points):
    d = points[:, None, :] - points[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def planted_frames(rng, sizes, n_atoms=8, noise=0.02, separation=1.5):
    """((M, n_atoms, 3) frames, planted labels): noisy copies of one distinct shape per group, shuffled."""
    frames, lab = [], []
    for g, m in enumerate(sizes):
        shape = separation * rng.standard_normal((n_atoms, 3))
        frames.append(shape[None] + noise * rng.standard_normal((m, n_atoms, 3)))
        lab += [g] * m
    order = rng.permutation(len(lab))
    return np.concatenate(frames)[order], np.array(lab)[order]
