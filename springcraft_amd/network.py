"""
Correlation networks on the device: the weighted residue graph of a coupling map, the shortest communication path between
every pair of residues, and which residues carry those paths.

No reference counterpart.  This is the second half of the workflows the coupling maps are computed for (Bio3D ``nma ->
dccm / lmi -> cna``, Sethi et al. 2009, WISP): what otherwise means copying every (N, N) map to the host and running a graph
library once per member.  Here the maps stay where ``dcc`` / ``generalized_correlation`` / ``prs`` left them, in the packed
pair layout of the batch solvers, and one set of kernels (``csrc/corr_network.hip``) serves one map, a uniform batch and a
ragged batch:

    edge weight      ``W[a, c] = -log(min(|c_ac|, 1))`` where ``|c_ac| >= min_correlation`` and, with coordinates, a and c are
                     within ``contact_cutoff``; ``+inf`` (no edge) elsewhere; 0 on the diagonal
    shortest paths   blocked Floyd-Warshall in float64 with a next-hop matrix, ``2 n^3`` additions and comparisons per member
    path usage       for every node the number of stored shortest paths through it

One path is stored per pair -- the first strict improvement in ascending pivot order -- so on ties :meth:`CorrelationNetwork.usage`
is NOT Brandes' fractional betweenness, which splits a pair's weight over all its shortest paths; on a graph without ties
(a tree, generic real weights) the two agree.  Not built: suboptimal paths, community detection, fractional betweenness,
a lower-triangle-only form for symmetric input.
"""

import ctypes as C

import numpy as np

from . import _hip

__all__ = ["CorrelationNetwork", "correlation_network", "shortest_paths", "network_of_weights", "USAGE_MAX_NODES"]

#: largest member :meth:`CorrelationNetwork.usage` takes: a target's next hops and counters are held in LDS
USAGE_MAX_NODES = 8192
_MAX_NODES = 262144
_MAX_MEMBERS = 65535


def check_network_args(min_correlation, contact_cutoff, has_coord):
    """
    ValueError for a ``min_correlation`` outside [0, 1], a ``contact_cutoff`` that is not positive, and a cutoff without
    coordinates or coordinates without a cutoff; host arithmetic only.  Returns ``(min_correlation, cutoff or None)`` as floats.
    """
    mc = float(min_correlation)
    if not 0.0 <= mc <= 1.0:
        raise ValueError(f"min_correlation must lie in [0, 1], got {min_correlation}")
    if contact_cutoff is None:
        if has_coord:
            raise ValueError("coord was given without a contact_cutoff")
        return mc, None
    cut = float(contact_cutoff)
    if not cut > 0.0 or not np.isfinite(cut):
        raise ValueError(f"contact_cutoff must be positive and finite, got {contact_cutoff}")
    if not has_coord:
        raise ValueError("a contact_cutoff needs the coordinates: pass coord")
    return mc, cut


def check_sizes(sizes):
    """ValueError for member sizes the kernels do not take; returns them as a list of ints."""
    sizes = [int(n) for n in sizes]
    if not sizes:
        raise ValueError("no members")
    if len(sizes) > _MAX_MEMBERS:
        raise ValueError(f"at most {_MAX_MEMBERS} members, got {len(sizes)}")
    if min(sizes) < 1 or max(sizes) > _MAX_NODES:
        raise ValueError(f"every member needs 1..{_MAX_NODES} nodes, got {min(sizes)}..{max(sizes)}")
    return sizes


def member_records(sizes):
    """(count, 3) int64: per member its size, the offset of its block in a packed pair buffer and of its first node."""
    n = np.asarray(sizes, dtype=np.int64)
    rec = np.zeros((len(n), 3), dtype=np.int64)
    rec[:, 0] = n
    rec[1:, 1] = np.cumsum(n * n)[:-1]
    rec[1:, 2] = np.cumsum(n)[:-1]
    return rec


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Form:
    """How the caller's maps map to the packed buffers and back: one (n, n) map, a (batch, n, n) stack or a list of maps."""

    def __init__(self, sizes, kind, host):
        self.sizes, self.kind, self.host = sizes, kind, host   # kind: "single" / "uniform" / "ragged"
        self.sq_off = [0] + [int(x) for x in np.cumsum(np.asarray(sizes, dtype=np.int64) ** 2)]
        self.node_off = [0] + [int(x) for x in np.cumsum(sizes)]

    def _out(self, t):
        return t.cpu().numpy() if self.host else t

    def pairs(self, buf):
        n = self.sizes[0]
        if self.kind == "single":
            return self._out(buf.view(n, n))
        if self.kind == "uniform":
            return self._out(buf.view(len(self.sizes), n, n))
        return [self._out(buf[self.sq_off[b]: self.sq_off[b + 1]].view(m, m)) for b, m in enumerate(self.sizes)]

    def nodes(self, buf):
        if self.kind == "single":
            return self._out(buf)
        if self.kind == "uniform":
            return self._out(buf.view(len(self.sizes), self.sizes[0]))
        return [self._out(buf[a:b]) for a, b in zip(self.node_off, self.node_off[1:])]


class CorrelationNetwork:
    """
    The communication network of one coupling map or of a batch of them, made by :func:`correlation_network`, a batch
    solver's ``correlation_network()`` or :func:`nma.correlation_network <springcraft_amd.nma.correlation_network>`.

    ``weights``, ``distances`` (float64) and ``next_hop`` (int32) have the form of the input: (n, n) for one map, (batch, n,
    n) for a stack, a list of (n_b, n_b) views of one packed buffer for a ragged batch; CUDA tensors, or NumPy arrays when
    the network was built from NumPy arrays.  ``next_hop[a, c]`` is the node after a on the stored shortest path to c, a on
    the diagonal and -1 exactly where ``distances[a, c]`` is ``+inf``.  ``flags`` (members,) int32 is non-zero for a member
    without a defined result -- a NaN in its map or coordinates, a NaN or negative weight: its distances are NaN, its
    next hops -1, its usage -1 and its betweenness NaN, and no other member is touched.  A member's bits do not depend on
    the batch, its position or its neighbours; a symmetric map gives distances equal to their transpose bit for bit.
    """

    def __init__(self, torch, device, ctx, form, rec, weights, flags, keep=()):
        self.torch, self.device, self.ctx, self._L = torch, device, ctx, _hip.lib()
        self._form, self._rec, self._w, self._flags, self._keep = form, rec, weights, flags, keep
        self._usage = None
        sizes = form.sizes
        with torch.cuda.device(device):
            self._d = torch.empty(weights.shape, dtype=torch.float64, device=device)
            self._s = torch.empty(weights.shape, dtype=torch.int32, device=device)
            ctx.check(self._L.sc_dev_net_paths_f64(ctx.handle, _p(rec), len(sizes), max(sizes), _p(weights), _p(self._d),
                                                   _p(self._s), _p(flags)))
        if form.host:
            ctx.synchronize()
        self.weights, self.distances, self.next_hop = form.pairs(self._w), form.pairs(self._d), form.pairs(self._s)

    @property
    def sizes(self):
        """Nodes per member."""
        return list(self._form.sizes)

    @property
    def flags(self):
        return self._form._out(self._flags)

    def _member(self, member, *nodes):
        sizes = self._form.sizes
        b = int(member)
        if not 0 <= b < len(sizes):
            raise IndexError(f"member {member} is out of bounds for a network of {len(sizes)} members")
        for v in nodes:
            if not 0 <= int(v) < sizes[b]:
                raise IndexError(f"node {v} is out of bounds for member {b} with {sizes[b]} nodes")
        lo, n = self._form.sq_off[b], sizes[b]
        return lo, n

    def path(self, a, c, member=0):
        """
        The stored shortest path from node a to node c of ``member`` as a list of node indices, ``[a, ..., c]``; ``[a]`` for
        ``a == c`` and ``[]`` when c cannot be reached (also in a flagged member).  Reads one column of ``next_hop``.
        """
        lo, n = self._member(member, a, c)
        a, c = int(a), int(c)
        col = self._s.view(-1)[lo: lo + n * n].view(n, n)[:, c].cpu().numpy()
        nodes, v = [a], a
        while v != c:
            v = int(col[v])
            if v < 0 or len(nodes) >= n:
                return []
            nodes.append(v)
        return nodes

    def path_length(self, a, c, member=0):
        """``distances[a, c]`` of ``member`` as a float: the sum of the edge weights along :meth:`path`, ``inf`` if there is none."""
        lo, n = self._member(member, a, c)
        return float(self._d.view(-1)[lo + int(a) * n + int(c)])

    def _usage_packed(self):
        if self._usage is None:
            torch, sizes = self.torch, self._form.sizes
            if max(sizes) > USAGE_MAX_NODES:
                raise ValueError(f"path usage takes members of at most {USAGE_MAX_NODES} nodes, got {max(sizes)}")
            with torch.cuda.device(self.device):
                out = torch.empty((self._form.node_off[-1],), dtype=torch.int64, device=self.device)
                self.ctx.check(self._L.sc_dev_net_usage(self.ctx.handle, _p(self._rec), len(sizes), max(sizes),
                                                        self._form.sq_off[-1], _p(self._s), _p(out), _p(self._flags)))
            if self._form.host:
                self.ctx.synchronize()
            self._usage = out
        return self._usage

    @property
    def usage(self):
        """
        int64, (n,) / (batch, n) / a list of (n_b,): for node v the number of ordered pairs (a, t) with a, t and v distinct
        and t reachable from a whose stored path passes through v.  Computed on first use.  One path per pair: on ties
        this is not Brandes' fractional count.  -1 for a flagged member.  Members above ``USAGE_MAX_NODES`` nodes raise
        ValueError.
        """
        return self._form.nodes(self._usage_packed())

    def betweenness(self, normalized=True):
        """
        Node betweenness from :attr:`usage` as float64, divided by ``(n - 1)(n - 2)``, the ordered pairs a node can lie
        between, when ``normalized``; 0 for a member of fewer than three nodes, NaN for a flagged member.  On a graph
        without ties this is ``networkx.betweenness_centrality`` of the directed graph; on ties it counts the stored path
        only (see :attr:`usage`).
        """
        torch = self.torch
        u = self._usage_packed()
        val = u.to(torch.float64)
        if normalized:
            n = np.repeat(np.asarray(self._form.sizes, dtype=np.float64), self._form.sizes)
            val = val / torch.from_numpy(np.maximum((n - 1) * (n - 2), 1.0)).to(self.device)   # (n < 3: usage is 0)
        val = torch.where(u < 0, torch.full_like(val, float("nan")), val)
        return self._form.nodes(val)

    def reachable(self):
        """Boolean, in the form of ``distances``: whether c can be reached from a (all False for a flagged member)."""
        return self._form.pairs(self._d < float("inf"))


def _open(device):
    """(torch, torch.device, context on the current stream of that device)."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) \
        if not isinstance(device, torch.device) else device
    return torch, dev, _hip.Context(dev.index, stream=torch.cuda.current_stream(dev).cuda_stream)


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _square(shape, what):
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] < 1:
        raise ValueError(f"Expected square {what}, got shape {tuple(shape)}")
    return int(shape[0])


def _pack_maps(maps, what, device):
    """
    (packed float64 CUDA tensor, :class:`_Form`, torch, device, ctx) of ``maps``: an (n, n) or (batch, n, n) NumPy array or
    CUDA tensor, or a list of square ones (a ragged batch).  Shapes are checked before a device is touched.
    """
    if isinstance(maps, (list, tuple)):
        if not maps:
            raise ValueError(f"no {what}")
        tensors = [_is_tensor(m) for m in maps]
        if any(tensors) != all(tensors):
            raise ValueError(f"{what}: NumPy arrays and tensors cannot be mixed")
        host = not tensors[0]
        items = [np.asarray(m, dtype=np.float64) for m in maps] if host else list(maps)
        sizes = check_sizes([_square(m.shape, what) for m in items])
        kind = "ragged"
    else:
        host = not _is_tensor(maps)
        items = np.asarray(maps, dtype=np.float64) if host else maps
        if items.ndim == 2:
            sizes, kind = check_sizes([_square(items.shape, what)]), "single"
        elif items.ndim == 3 and items.shape[0] >= 1:
            sizes, kind = check_sizes([_square(items.shape[1:], what)] * int(items.shape[0])), "uniform"
        else:
            raise ValueError(f"Expected {what} of shape (n, n) or (batch, n, n), got {tuple(items.shape)}")
    if host:
        torch, dev, ctx = _open(device)
        flat = np.concatenate([m.reshape(-1) for m in items]) if kind == "ragged" else np.ascontiguousarray(items).reshape(-1)
        with torch.cuda.device(dev):
            buf = torch.from_numpy(np.array(flat, dtype=np.float64)).to(dev)
    else:
        first = items[0] if kind == "ragged" else items
        for m in (items if kind == "ragged" else [items]):
            if not m.is_cuda or m.dtype != first.dtype or m.device != first.device:
                raise ValueError(f"{what} must be CUDA float64 tensors on one device")
        torch, dev, ctx = _open(first.device)
        if first.dtype != torch.float64:
            raise ValueError(f"{what} must be float64, got {first.dtype}")
        with torch.cuda.device(dev):
            buf = torch.cat([m.reshape(-1) for m in items]) if kind == "ragged" else items.contiguous().view(-1)
    return buf, _Form(sizes, kind, host), torch, dev, ctx


def _pack_coord(coord, form, torch, dev):
    """The packed (sum n, 3) coordinates of the members, in the form of the maps."""
    total = form.node_off[-1]
    if form.kind == "ragged" and isinstance(coord, (list, tuple)):
        if len(coord) != len(form.sizes):
            raise ValueError(f"{len(coord)} coordinate sets were given for {len(form.sizes)} maps")
        parts = [c if _is_tensor(c) else torch.from_numpy(np.array(c, dtype=np.float64)) for c in coord]
        for c, n in zip(parts, form.sizes):
            if tuple(c.shape) != (n, 3):
                raise ValueError(f"Expected coordinates of shape ({n}, 3), got {tuple(c.shape)}")
        packed = torch.cat([c.to(dev, torch.float64) for c in parts])
    else:
        c = coord if _is_tensor(coord) else torch.from_numpy(np.array(coord, dtype=np.float64))
        want = {"single": (form.sizes[0], 3), "uniform": (len(form.sizes), form.sizes[0], 3), "ragged": (total, 3)}[form.kind]
        if tuple(c.shape) != want:
            raise ValueError(f"Expected coordinates of shape {want}, got {tuple(c.shape)}")
        packed = c.to(dev, torch.float64).contiguous().view(total, 3)
    return packed


def _upload_records(torch, dev, sizes):
    # through page-locked memory: a copy from pageable memory would make the host wait for the stream
    return torch.from_numpy(member_records(sizes)).pin_memory().to(dev, non_blocking=True)


def network_from_packed(torch, dev, ctx, form, corr, coord, cutoff, min_correlation, keep=()):
    """
    :class:`CorrelationNetwork` of the packed coupling maps ``corr`` (``form``: how they are handed back) and the packed
    coordinates ``coord`` or None; the arguments were checked (:func:`check_network_args`).  Only enqueues.
    """
    L = _hip.lib()
    sizes = form.sizes
    with torch.cuda.device(dev):
        rec = _upload_records(torch, dev, sizes)
        w = torch.empty(corr.shape, dtype=torch.float64, device=dev)
        flags = torch.empty((len(sizes),), dtype=torch.int32, device=dev)
        cut_sq = 0.0 if cutoff is None else float(np.float64(cutoff) ** 2)
        ctx.check(L.sc_dev_net_weights_f64(ctx.handle, _p(rec), len(sizes), max(sizes), _p(corr), _p(coord), cut_sq,
                                           float(min_correlation), _p(w), _p(flags)))
    return CorrelationNetwork(torch, dev, ctx, form, rec, w, flags, keep=(corr, coord) + tuple(keep))


def correlation_network(corr, coord=None, contact_cutoff=None, min_correlation=0.0, device=None):
    """
    The :class:`CorrelationNetwork` of coupling maps: ``corr`` an (n, n) or (batch, n, n) NumPy array or CUDA float64 tensor
    (``dcc(norm=True)``, ``generalized_correlation()``, a normalised ``prs`` -- any map with entries in [-1, 1]; it need not
    be symmetric), or a list of square maps of different sizes.  An edge a - c exists where ``|corr[a, c]| >=
    min_correlation`` and, with ``coord`` ((n, 3), (batch, n, 3), or for a list the (sum n, 3) packed array or a list) and
    ``contact_cutoff``, the two are within the cutoff; its weight is ``-log(min(|corr[a, c]|, 1))``.  NumPy arrays in give
    NumPy arrays out; ``device`` chooses the GPU for them.

    ValueError before anything is enqueued: ``min_correlation`` outside [0, 1], a cutoff that is not positive, a cutoff
    without coordinates or the reverse, maps that are not square.
    """
    mc, cut = check_network_args(min_correlation, contact_cutoff, coord is not None)
    buf, form, torch, dev, ctx = _pack_maps(corr, "correlation maps", device)
    with torch.cuda.device(dev):
        xyz = None if coord is None else _pack_coord(coord, form, torch, dev)
    return network_from_packed(torch, dev, ctx, form, buf, xyz, cut, mc)


def shortest_paths(weights, device=None):
    """
    ``(distances, next_hop)`` of the non-negative edge weights ``weights``, in the forms :func:`correlation_network` takes;
    ``+inf`` is "no edge", the matrix may be asymmetric (a directed network), the diagonal is taken as 0.  See
    :class:`CorrelationNetwork` for the two results; a member with a NaN or negative weight comes back as NaN / -1.
    NumPy arrays in give NumPy arrays out.
    """
    net = network_of_weights(weights, device)
    return net.distances, net.next_hop


def network_of_weights(weights, device=None):
    """The :class:`CorrelationNetwork` of given edge weights (:func:`shortest_paths` with the object kept, for ``usage``)."""
    buf, form, torch, dev, ctx = _pack_maps(weights, "edge weights", device)
    with torch.cuda.device(dev):
        rec = _upload_records(torch, dev, form.sizes)
        flags = torch.zeros((len(form.sizes),), dtype=torch.int32, device=dev)
    return CorrelationNetwork(torch, dev, ctx, form, rec, buf, flags)
