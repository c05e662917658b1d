"""
Clustering on the device: the items of a square dissimilarity matrix -- the conformers of an ensemble by their pairwise
RMSD (:meth:`Ensemble.rmsd_matrix <springcraft_amd.Ensemble.rmsd_matrix>`), the residues of a correlation network by its
path lengths, ``1 - |dcc|`` -- put into groups with a representative each.

No reference counterpart.  This is the step every comparable package takes from the matrix (Bio3D ``rmsd -> hclust /
cutree``, GROMACS ``gmx cluster -method gromos``, ProDy's ClustENM, k-medoids on the RMSD matrix in MDTraj / MDAnalysis), and
what otherwise means copying an (M, M) float64 matrix to the host.  Here the matrix stays where it was computed and two
methods run on it as dependent rounds of whole-matrix passes (``csrc/cluster.hip``):

    :func:`cluster_gromos`    neighbour-count clustering (Daura et al. 1999): the item with the most neighbours within
                              ``cutoff`` and its neighbours form a cluster and leave; repeat on the rest
    :func:`cluster_kmedoids`  PAM: BUILD, then best-swap SWAP with the FastPAM1 evaluation (Schubert & Rousseeuw 2021)

Item i is invalid when ``dist[i, i]`` is NaN (what ``rmsd_matrix`` writes for a non-finite frame): label -1, it neither
counts nor is counted and is never a representative.  A NaN between two valid items sets ``flag``: every label is -1 and
there are no clusters.  An item is always its own neighbour.  Ties go to the lowest index, two calls agree bit for bit.
Kernels enqueue; the host reads four int32 every ``check_every`` rounds and nothing else comes back.

:func:`cluster_gromos_frames` (and ``Ensemble.cluster(..., matrix_free=True)``) is the matrix-free form of the first: the
RMSD product kernel writes ``rmsd <= cutoff`` as bits straight into the run's workspace (``csrc/rmsd_matrix.hip``) and the
(M, M) float64 matrix is never stored, 64 times less memory; the rounds are the same.

Not built: hierarchical linkage, silhouettes, batches of matrices, matrix-free k-medoids (PAM reads ``dist`` in every pass).
"""

import ctypes as C

import numpy as np

from . import _hip

__all__ = ["Clustering", "cluster_gromos", "cluster_gromos_frames", "cluster_kmedoids", "MAX_ITEMS", "MAX_MEDOIDS"]

#: the limits of ``csrc/cluster_policy.h``: an item is an int32 and a row a workgroup; a row's per-slot sums are held in LDS
MAX_ITEMS = 262144
MAX_MEDOIDS = 1024


# ---- host-side argument checks (before any device call) -----------------------------------------------------------------
def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def check_matrix(dist):
    """``(n, host)`` of a square float64 matrix, a NumPy array (``host``) or a CUDA tensor; ValueError for anything else."""
    host = not _is_tensor(dist)
    if host:
        if not isinstance(dist, np.ndarray):
            raise ValueError(f"dist must be a NumPy array or a CUDA tensor, got {type(dist).__name__}")
        if dist.dtype != np.float64:
            raise ValueError(f"dist must be float64, got {dist.dtype}")
    else:
        if str(dist.dtype) != "torch.float64":
            raise ValueError(f"dist must be float64, got {dist.dtype}")
        if not dist.is_cuda:
            raise ValueError("dist must be a NumPy array or a CUDA tensor")
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1] or dist.shape[0] < 1:
        raise ValueError(f"Expected a square dissimilarity matrix, got shape {tuple(dist.shape)}")
    return int(dist.shape[0]), host


def check_gromos_args(n, cutoff, max_clusters, check_every):
    """``(cutoff, max_clusters or None, check_every)`` checked: host arithmetic only."""
    if cutoff is None:
        raise ValueError("neighbour-count clustering needs a cutoff")
    cut = float(cutoff)
    if not cut >= 0.0 or not np.isfinite(cut):
        raise ValueError(f"cutoff must be finite and not negative, got {cutoff}")
    if max_clusters is not None:
        max_clusters = int(max_clusters)
        if max_clusters < 1:
            raise ValueError(f"max_clusters must be at least 1, got {max_clusters}")
        max_clusters = min(max_clusters, n)
    if int(check_every) < 1:
        raise ValueError(f"check_every must be at least 1, got {check_every}")
    return cut, max_clusters, int(check_every)


def check_kmedoids_args(n, k, max_iter, check_every):
    """``(k, max_iter, check_every)`` checked: host arithmetic only."""
    if k is None:
        raise ValueError("k-medoids needs k")
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"k must lie in 1..{n}, got {k}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")
    if int(check_every) < 1:
        raise ValueError(f"check_every must be at least 1, got {check_every}")
    return k, int(max_iter), int(check_every)


def workspace_bytes(n, k):
    """Bytes of the workspace of a run (``k`` 0: neighbour count); ValueError for a size the kernels cannot index."""
    size = int(_hip.lib().sc_cluster_workspace(int(n), int(k)))
    if size < 0:
        raise ValueError(f"clustering takes at most {MAX_ITEMS} items and {MAX_MEDOIDS} medoids, got {n} items"
                         + (f" and k = {k}" if k else ""))
    return size


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Clustering:
    """
    The result of :func:`cluster_gromos` / :func:`cluster_kmedoids`: CUDA tensors, or NumPy arrays when the matrix was one.

    ``labels`` (M,) int32: the cluster of every item, -1 for an invalid item (and for what ``max_clusters`` left over);
    ``representatives`` (n_clusters,) int32: the centres or medoids; ``sizes`` (n_clusters,) int32; ``n_clusters``; ``flag``
    (1: a NaN between two valid items, nothing else is defined).  k-medoids also: ``total_deviation`` (iterations + 1,) float64,
    the sum of every item's distance to its medoid after BUILD and after every accepted swap; ``iterations``; ``converged``.
    ``method`` is ``"gromos"`` or ``"kmedoids"``.  What needs the status is read from the device on first use;
    ``status_reads`` counts those reads, the driver's included.
    """

    def __init__(self, method, torch, ctx, host, labels, reps, sizes, status, td=None, keep=()):
        self.method, self.torch, self.ctx, self._host = method, torch, ctx, host
        self._labels, self._reps, self._sizes, self._status, self._td, self._keep = labels, reps, sizes, status, td, keep
        self._st = None
        self.status_reads = 0

    def _read_status(self):
        """The four status words on the host: waits for the stream."""
        self._st = [int(x) for x in self._status.cpu().tolist()]
        self.status_reads += 1
        return self._st

    def _final(self):
        return self._st if self._st is not None else self._read_status()

    def _out(self, t):
        return t.cpu().numpy() if self._host else t

    @property
    def flag(self):
        return self._final()[2]

    @property
    def n_clusters(self):
        st = self._final()
        if st[2]:
            return 0
        return st[1] if self.method == "gromos" else st[3]

    @property
    def labels(self):
        return self._out(self._labels)

    @property
    def representatives(self):
        return self._out(self._reps[: self.n_clusters])

    @property
    def sizes(self):
        return self._out(self._sizes[: self.n_clusters])

    @property
    def iterations(self):
        """k-medoids: the swaps accepted (None for neighbour-count clustering)."""
        return None if self._td is None else self._final()[1]

    @property
    def converged(self):
        """k-medoids: whether SWAP ended because no swap lowers the total deviation (None for neighbour-count clustering)."""
        return None if self._td is None else self._final()[0] == 0

    @property
    def total_deviation(self):
        if self._td is None:
            return None
        st = self._final()
        return self._out(self._td[: 0 if st[2] else st[1] + 1])

    def members(self, c):
        """The indices of cluster ``c``, ascending, int64."""
        c = int(c)
        if not 0 <= c < self.n_clusters:
            raise IndexError(f"cluster {c} is out of bounds for {self.n_clusters} clusters")
        return self._out(self.torch.nonzero(self._labels == c).view(-1))


def _open(dist, host, device):
    """(torch, device, context on the current stream, the matrix as a contiguous CUDA tensor)."""
    import torch

    if host:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    else:
        dev = dist.device
        if device is not None and dev.index != int(device):
            raise ValueError(f"dist is on {dev}, the clustering was asked for device {int(device)}")
    ctx = _hip.Context(dev.index, stream=torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if host:
            a = np.ascontiguousarray(dist)
            mat = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)   # (torch wraps writable arrays only)
        else:
            mat = dist.contiguous()
    return torch, dev, ctx, mat


def cluster_gromos(dist, cutoff, max_clusters=None, check_every=32, device=None):
    """
    Neighbour-count clustering of the (M, M) float64 dissimilarity matrix ``dist`` (NumPy array or CUDA tensor).  Until no
    item is left: every remaining item counts the remaining items within ``cutoff`` of it (``dist[i, j] <= cutoff`` along
    its row, itself included); the one with the most, the lowest index among equals, becomes the centre of the next
    cluster, which takes those neighbours.  Sizes come out non-increasing; a cutoff of 0 groups exact duplicates.

    One streaming pass packs ``dist <= cutoff`` into a bit matrix, M^2 / 8 bytes, and the rounds run on that.  The host
    enqueues ``check_every`` rounds and reads the status, until nothing is left.  With ``max_clusters`` exactly that many
    rounds are enqueued and nothing is read: the call returns at once, what is left over keeps label -1.

    ValueError before any device work: a matrix that is not square or not float64, a cutoff that is negative or not finite,
    ``max_clusters`` or ``check_every`` below 1, more than ``MAX_ITEMS`` items.
    """
    n, host = check_matrix(dist)
    cut, max_clusters, check_every = check_gromos_args(n, cutoff, max_clusters, check_every)
    size = workspace_bytes(n, 0)
    torch, dev, ctx, mat = _open(dist, host, device)

    def init(ws, labels, status):
        ctx.check(_hip.lib().sc_dev_cluster_gromos_init_f64(ctx.handle, _p(mat), n, cut, _p(ws), size, _p(labels), _p(status)))

    out = _gromos_run(torch, dev, ctx, host, n, size, max_clusters, check_every, init, keep=(mat,))
    if host:
        ctx.synchronize()
    return out


def _gromos_run(torch, dev, ctx, host, n, size, max_clusters, check_every, init, keep=()):
    """
    A neighbour-count run of ``n`` items whose workspace ``init(ws, labels, status)`` fills, from a stored matrix
    (:func:`cluster_gromos`) or from the frames (:func:`cluster_gromos_frames`): the buffers, the rounds in chunks of
    ``check_every`` with one status read each, or exactly ``max_clusters`` rounds and no read.  Arguments checked already.
    """
    L = _hip.lib()
    cap = n if max_clusters is None else max_clusters
    with torch.cuda.device(dev):
        ws = torch.empty((size,), dtype=torch.uint8, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        reps = torch.empty((cap,), dtype=torch.int32, device=dev)
        sizes = torch.empty((cap,), dtype=torch.int32, device=dev)
        status = torch.empty((4,), dtype=torch.int32, device=dev)
        out = Clustering("gromos", torch, ctx, host, labels, reps, sizes, status, keep=tuple(keep) + (ws,))
        init(ws, labels, status)

        def rounds(count):
            ctx.check(L.sc_dev_cluster_gromos_rounds(ctx.handle, n, count, cap, _p(ws), size, _p(labels), _p(reps),
                                                     _p(sizes), _p(status)))

        if max_clusters is not None:
            rounds(max_clusters)
        else:
            done = 0
            while done < n:   # (a round removes its centre at least: n rounds always suffice)
                rounds(min(check_every, n - done))
                done += min(check_every, n - done)
                if out._read_status()[0] == 0:
                    break
    return out


def check_frame_counts(n_frames, n_atoms):
    """ValueError for more frames than clustering takes, or frames the RMSD product cannot index: host arithmetic only."""
    workspace_bytes(n_frames, 0)
    if int(_hip.lib().sc_rmsd_matrix_workspace(int(n_frames), 0, int(n_atoms))) < 0:
        raise ValueError(f"{n_frames} frames of {n_atoms} atoms are beyond the kernels' index range")


def gromos_from_frames(ens, cutoff, fit=True, squared=False, max_clusters=None, check_every=32, host=False):
    """
    Neighbour-count clustering of the frames of the :class:`~springcraft_amd.Ensemble` ``ens`` without the RMSD matrix:
    the product kernel fills the run's workspace with the neighbour bits (``sc_dev_frame_neighbours_init_f64``), then the
    rounds of :func:`cluster_gromos`.  A :class:`Clustering` of CUDA tensors (``host``: of NumPy arrays).
    """
    n = ens.n_frames
    cut, max_clusters, check_every = check_gromos_args(n, cutoff, max_clusters, check_every)
    check_frame_counts(n, ens.n_atoms)
    size = workspace_bytes(n, 0)
    flags = (1 if fit else 0) | (2 if squared else 0)

    def init(ws, labels, status):
        ens.ctx.check(_hip.lib().sc_dev_frame_neighbours_init_f64(ens.ctx.handle, _p(ens.frames), n, ens.n_atoms, _p(ens._w),
                                                                  flags, cut, _p(ws), size, _p(labels), _p(status)))

    return _gromos_run(ens.torch, ens.device, ens.ctx, host, n, size, max_clusters, check_every, init, keep=(ens.frames, ens._w))


def cluster_gromos_frames(coords, cutoff, weights=None, fit=True, squared=False, max_clusters=None, check_every=32, device=None):
    """
    Neighbour-count clustering of the frames ``coords`` (M, N, 3) by their pairwise RMSD, matrix-free: host arrays in, a
    :class:`Clustering` of NumPy arrays out, like ``rmsd_matrix(coords, ...)`` followed by :func:`cluster_gromos` on its
    result, with the same labels, centres and sizes, but the (M, M) float64 matrix is never stored: the device holds
    M^2 / 8 bytes of neighbour bits instead of 8 M^2, so ``MAX_ITEMS`` frames fit where 60 000 did.  ``weights``, ``fit``
    and ``squared`` as in :meth:`Ensemble.rmsd_matrix <springcraft_amd.Ensemble.rmsd_matrix>`; ``cutoff`` in the value's
    units.

    ValueError before any device work: coordinates that are not (M, N, 3), a cutoff that is negative or not finite, weights
    that are negative or not finite, ``max_clusters`` or ``check_every`` below 1, more than ``MAX_ITEMS`` frames.
    """
    from . import ensemble as _ensemble

    a = _ensemble._host_frames(coords)
    w = _ensemble._checked_weights(weights, a.shape[1])
    check_gromos_args(a.shape[0], cutoff, max_clusters, check_every)
    check_frame_counts(a.shape[0], a.shape[1])
    ens = _ensemble.Ensemble(a, weights=w, device=device)
    out = gromos_from_frames(ens, cutoff, fit=fit, squared=squared, max_clusters=max_clusters, check_every=check_every,
                             host=True)
    ens.ctx.synchronize()
    return out


def cluster_kmedoids(dist, k, max_iter=100, check_every=4, device=None):
    """
    k-medoids (PAM) of the (M, M) float64 dissimilarity matrix ``dist`` (NumPy array or CUDA tensor).  BUILD places the
    medoids one by one: first the item with the smallest sum of its row, then always the item that lowers the total
    deviation -- the sum of every item's distance to its nearest medoid -- the most; k passes over ``dist``.  SWAP, one pass
    per iteration, evaluates every (candidate, medoid) exchange, applies the best one while it lowers the total deviation
    and has converged when none does.  The host enqueues ``check_every`` iterations and reads the status, ``max_iter``
    iterations at the most: running out returns what there is with ``converged = False``.

    An item's label is the slot of its nearest medoid along the medoid's row, the lowest slot among equals.  With k = 1
    there is no SWAP; with k at or above the number of valid items every valid item is a medoid.

    ValueError before any device work: a matrix that is not square or not float64, k outside 1..M, ``max_iter`` or
    ``check_every`` below 1, more than ``MAX_ITEMS`` items or ``MAX_MEDOIDS`` medoids.
    """
    n, host = check_matrix(dist)
    k, max_iter, check_every = check_kmedoids_args(n, k, max_iter, check_every)
    size = workspace_bytes(n, k)
    torch, dev, ctx, mat = _open(dist, host, device)
    L = _hip.lib()
    td_cap = max_iter + 1
    with torch.cuda.device(dev):
        ws = torch.empty((size,), dtype=torch.uint8, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        reps = torch.empty((k,), dtype=torch.int32, device=dev)
        sizes = torch.empty((k,), dtype=torch.int32, device=dev)
        td = torch.zeros((td_cap,), dtype=torch.float64, device=dev)
        status = torch.empty((4,), dtype=torch.int32, device=dev)
        out = Clustering("kmedoids", torch, ctx, host, labels, reps, sizes, status, td=td, keep=(mat, ws))
        ctx.check(L.sc_dev_cluster_kmedoids_init_f64(ctx.handle, _p(mat), n, k, _p(ws), size, _p(labels), _p(reps), _p(sizes),
                                                     _p(td), td_cap, _p(status)))
        done = 0
        while k > 1 and done < max_iter:
            count = min(check_every, max_iter - done)
            ctx.check(L.sc_dev_cluster_kmedoids_swaps_f64(ctx.handle, _p(mat), n, k, count, _p(ws), size, _p(labels),
                                                          _p(reps), _p(sizes), _p(td), td_cap, _p(status)))
            done += count
            st = out._read_status()
            if st[0] == 0 or st[2]:
                break
    if host:
        ctx.synchronize()
    return out
