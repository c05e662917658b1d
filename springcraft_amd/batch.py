"""
Batched-structure axis: many independent ANM / GNM solves per GPU, sharded over the GPUs of a node.

The reference has no batch axis (one model object = one structure, anm.py:62-63); this module adds
the one parallel axis the path offers — independent structures — in the shape BASELINE.json's
north star asks for: structures are partitioned over ranks (one process per GPU), every rank
assembles and eigendecomposes its shard with the batched device entry points
(``sc_dev_hessian_f64`` / ``sc_dev_eigh_f64``), and RCCL (``torch.distributed`` backend ``nccl``) is
used only to scatter coordinates from / gather eigenvalues to the root rank.  There is no
collective inside the data path.

torch is used strictly as plumbing: device buffers, the stream handed to the C ABI, and the
process group.
"""

import ctypes as C

import numpy as np

from . import _hip
from .forcefield import device_plan

__all__ = ["DeviceBatchSolver", "RaggedBatchSolver", "shard_bounds", "solve_sharded", "partition_lpt", "size_buckets",
           "solve_ragged", "batch_mode_rows", "ragged_subset_plan"]

K_B = 1.380649e-23


def shard_bounds(n_items, world_size, rank):
    """Contiguous, balanced partition of ``n_items`` structures: rank r owns [lo, hi)."""
    base, rem = divmod(n_items, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def batch_mode_rows(mode_subset, ntriv, subset, m, window=None):
    """
    Rows of a batch solver's ``w`` / ``v`` for the GLOBAL ascending mode indices ``mode_subset`` (the reference's
    ``mode_subset``, nma.py:161-168): pure host arithmetic, checked before any device call.

    ntriv    trivial modes, 6 for an ANM, 1 for a GNM
    subset   None for a full-spectrum solver (row r is mode r) or its ``subset_by_index=(lo, hi)`` (row r is mode lo + r)
    m        matrix order
    window   the solver's ``subset_by_value`` or None; with a window the modes' indices are not known on the host, so
             ``mode_subset`` must be None and None is returned: the selection is the window itself

    ``mode_subset=None`` gives every solved mode with index >= ``ntriv``.  A trivial index raises the reference's
    ValueError (nma.py:164-166), an index that was not solved a ValueError naming the solved range.  Repeated and
    unsorted indices are kept as they are: each occurrence counts (NumPy fancy indexing, nma.py:167-168).
    Returns an int32 array of row numbers.
    """
    if window is not None:
        if mode_subset is not None:
            raise ValueError("mode_subset cannot be combined with subset_by_value: the solved modes are the eigenvalue "
                             "window, whose mode indices are only known on the device")
        return None
    lo, hi = (0, m - 1) if subset is None else (int(subset[0]), int(subset[1]))
    if mode_subset is None:
        return np.arange(max(ntriv, lo) - lo, hi - lo + 1, dtype=np.int32)
    idx = np.asarray(mode_subset)
    if idx.size and idx.dtype.kind not in "iu":
        raise IndexError("mode_subset must hold integer mode indices")
    idx = idx.astype(np.int64).reshape(-1)
    if np.any(idx < ntriv):
        raise ValueError("Trivial modes are included in the current selection. Please check your input.")
    if np.any(idx < lo) or np.any(idx > hi):
        bad = idx[(idx < lo) | (idx > hi)][0]
        raise ValueError(f"mode {bad} was not solved: this solver holds modes {lo}..{hi}")
    return (idx - lo).astype(np.int32)


def ragged_subset_plan(sizes, dim, subset_by_index=None, subset_by_value=None, max_modes=None):
    """
    What a :class:`RaggedBatchSolver` solves per slot, checked on the host before any device call.  A slot is
    ``diag(M, D)`` with the pad D above M's spectrum, so its lowest eigenpairs are the structure's own; a subset must stay
    inside the ``dim * min(sizes)`` modes that EVERY structure has, or the smallest one would return pads as modes.

    subset_by_index  None or (lo, hi), inclusive: needs ``0 <= lo <= hi < dim * min(sizes)``
    subset_by_value  None or (vl, vu) with ``max_modes = K``, ``1 <= K <= dim * min(sizes)``; the same mutual-exclusion
                     and ``max_modes`` rules as :class:`DeviceBatchSolver` (``nma._value_window``)

    Returns a dict: ``subset`` ((lo, hi) or None), ``window`` ((vl, vu) or None), ``max_modes`` (int or None), ``nvec``
    (rows of ``w`` / ``v`` per slot; None for the full spectrum, where it is the slot order), ``first_row`` (global mode
    index of row 0: lo, else 0) and ``row_limits`` (per structure, how many rows can be its own modes: ``dim * n_b`` for the
    full spectrum, else ``nvec``).
    """
    from .nma import _value_window

    sizes = [int(n) for n in sizes]
    dim = int(dim)
    if not sizes:
        raise ValueError("no structures")
    window = _value_window(subset_by_value, subset_by_index)
    if window is None and max_modes is not None:
        raise ValueError("max_modes applies to subset_by_value only")
    smallest = int(np.argmin(sizes))
    own_min = dim * sizes[smallest]
    whose = f"the smallest structure ({smallest}: {sizes[smallest]} atoms) has {own_min} modes"
    plan = {"subset": None, "window": window, "max_modes": None, "nvec": None, "first_row": 0,
            "row_limits": [dim * n for n in sizes]}
    if window is not None:
        if max_modes is None:
            raise ValueError("subset_by_value needs max_modes, the number of eigenpairs kept per structure")
        if not 1 <= int(max_modes) <= own_min:
            raise ValueError(f"max_modes {max_modes} outside 1..{own_min}: {whose}")
        k = int(max_modes)
        plan.update(max_modes=k, nvec=k, row_limits=[k] * len(sizes))
    elif subset_by_index is not None:
        lo, hi = int(subset_by_index[0]), int(subset_by_index[1])
        if not 0 <= lo <= hi < own_min:
            raise ValueError(f"subset_by_index {tuple(subset_by_index)} outside 0..{own_min - 1}: {whose}")
        plan.update(subset=(lo, hi), nvec=hi - lo + 1, first_row=lo, row_limits=[hi - lo + 1] * len(sizes))
    return plan


def _aniso_expand(solver, packed):
    """(..., 6) device tensor in ANISOU order -> (..., 3, 3): an index gather on the solver's device, enqueue only."""
    if getattr(solver, "_aniso_index", None) is None:
        from .nma import ANISOU_INDEX

        # (once per solver, through page-locked memory: later calls find the nine indices on the device)
        host = solver.torch.from_numpy(ANISOU_INDEX.reshape(-1).astype(np.int64)).pin_memory()
        solver._aniso_index = host.to(solver.device, non_blocking=True)
    return packed.index_select(-1, solver._aniso_index).view(*packed.shape[:-1], 3, 3)


def _effector_sensor(torch, prs):
    """Means of the off-diagonal entries of (..., N, N) PRS matrices along every row and every column (nma.py:527-569)."""
    n = prs.shape[-1]
    off = prs - torch.diag_embed(prs.diagonal(dim1=-2, dim2=-1))
    return off.sum(dim=-1) / (n - 1), off.sum(dim=-2) / (n - 1)


def _rmsip_pick(n_modes, mode_subset):
    """
    ``pick(solver)`` -> (sel, counts, device list) of :meth:`_BatchSolver.rmsip`'s selection on that solver: ``mode_subset``,
    else the first ``n_modes`` non-trivial solved modes, behind a window the window.
    """
    def pick(s):
        subset = mode_subset if (mode_subset is not None or s.window is not None) else s._first_modes(n_modes)
        sel, counts = s._selection(subset, pinv_default=False)
        return sel, counts, s._rows_keep

    return pick


def _listed_pick(mode_subset, pinv_default):
    """``pick(solver)`` -> (sel, counts, device list) of the selection :meth:`_BatchSolver.dcc` (``pinv_default``) / ``msf`` makes."""
    def pick(s):
        sel, counts = s._selection(mode_subset, pinv_default=pinv_default)
        return sel, counts, s._rows_keep

    return pick


def _trivial_rows(ntriv, first_row, nvec):
    """
    How many of a solver's ``nvec`` rows, row r being global mode ``first_row + r``, are trivial modes: the first row of
    the "every solved non-trivial mode" selection (``nvec``: there is none) and the rows :meth:`frequencies` takes ``abs`` of.
    """
    return min(max(ntriv - first_row, 0), nvec)


class _Layout:
    """
    Where the consumers' results of a batch lie in their buffers and how they are handed back: what differs between
    :class:`DeviceBatchSolver` (:class:`_UniformLayout`) and :class:`RaggedBatchSolver` (:class:`_RaggedLayout`).  Pure host
    arithmetic on shapes, no device context.  A layout answers:

    atoms_shape(tail)   shape of a per-atom result buffer with ``tail`` values per atom; also the shape ``coord``
                        (``tail=(3,)``) and ``atom_scale`` (``tail=()``) must have, and how error messages name it
    pairs_shape()       shape of a per-pair result buffer
    atoms_out(buf), pairs_out(buf), rows_out(t, single)
                        the caller's form of a per-atom / per-pair buffer and of a per-row (batch, [q,] nvec) tensor;
                        ``single``: the q axis holds the one vector that was given without it and is dropped
    pair_blocks(out, atom_scale)
                        (pairs, scale or None) blocks, the last two axes of ``pairs`` being (atom, atom), in which
                        ``pairs_out``'s result ``out`` is post-processed
    displacement()      (lead, tail, wording): a displacement has shape ``lead + tail`` or ``lead + (q,) + tail``
    vectors_shape(q), vectors_out(buf, single)
                        shape of a result buffer of q displacement-shaped vectors per structure, ``lead + (q,) + tail``,
                        and the caller's form of it; ``single`` as for ``rows_out``
    """

    def displacement_q(self, shape, what="displacement"):
        """
        (q, whether it is one vector without a q axis) of a displacement of ``shape``; ValueError for any other shape.
        ``what``: how the message names the vector (a force has a displacement's shapes).
        """
        lead, tail, names = self.displacement()
        shape = tuple(shape)
        if shape == lead + tail:
            return 1, True
        if len(shape) == len(lead) + 1 + len(tail) and shape[:len(lead)] == lead and shape[len(lead) + 1:] == tail:
            return shape[len(lead)], False
        raise ValueError(f"Expected a {what} of shape {names}, got {shape}")

    def vectors_shape(self, q):
        lead, tail, _ = self.displacement()
        return lead + (int(q),) + tail


class _UniformLayout(_Layout):
    """``batch`` structures of ``n_atoms`` atoms: every result is one tensor with a leading batch axis, handed back as it is."""

    ragged = False

    def __init__(self, batch, n_atoms, dim):
        self.batch, self.n_atoms, self.dim = int(batch), int(n_atoms), int(dim)

    def atoms_shape(self, tail=()):
        return (self.batch, self.n_atoms) + tuple(tail)

    def pairs_shape(self):
        return (self.batch, self.n_atoms, self.n_atoms)

    def atoms_out(self, buf):
        return buf

    pairs_out = atoms_out

    def rows_out(self, t, single=False):
        return t[:, 0] if single else t

    def vectors_out(self, buf, single=False):
        return buf[:, 0] if single else buf

    def pair_blocks(self, out, atom_scale):
        return [(out, atom_scale)]

    def displacement(self):
        names = "(batch, N, 3) or (batch, q, N, 3)" if self.dim == 3 else "(batch, N) or (batch, q, N)"
        tail = (self.n_atoms, 3) if self.dim == 3 else (self.n_atoms,)
        return (self.batch,), tail, f"{names} with batch = {self.batch}, N = {self.n_atoms}"


class _RaggedLayout(_Layout):
    """
    Structures of ``sizes`` atoms back to back in one packed buffer, handed back as a list of views: structure b's atoms
    start at ``atom_off[b] = sum(sizes[:b])``, its (n_b, n_b) block at ``sq_off[b] = sum(sizes[:b] ** 2)``, and of a per-row
    tensor it gets its first ``row_limits[b]`` rows (:func:`ragged_subset_plan`).
    """

    ragged = True

    def __init__(self, sizes, dim, row_limits):
        self.sizes, self.dim, self.row_limits = [int(n) for n in sizes], int(dim), [int(r) for r in row_limits]
        self.atom_off = [0] + [int(x) for x in np.cumsum(self.sizes)]
        self.sq_off = [0] + [int(x) for x in np.cumsum(np.asarray(self.sizes, dtype=np.int64) ** 2)]

    def atoms_shape(self, tail=()):
        return (self.atom_off[-1],) + tuple(tail)

    def pairs_shape(self):
        return (self.sq_off[-1],)

    def atoms_out(self, buf):
        return [buf[a:b] for a, b in zip(self.atom_off, self.atom_off[1:])]

    def pairs_out(self, buf):
        return [buf[self.sq_off[b]: self.sq_off[b + 1]].view(n, n) for b, n in enumerate(self.sizes)]

    def rows_out(self, t, single=False):
        return [t[b, 0, :r] if single else t[b, ..., :r] for b, r in enumerate(self.row_limits)]

    def vectors_out(self, buf, single=False):
        """``buf`` (q, sum(sizes)[, 3]) packed like the coordinates -> per structure the view (n_b[, 3]) or (q, n_b[, 3])."""
        return [buf[0, a:b] if single else buf[:, a:b] for a, b in zip(self.atom_off, self.atom_off[1:])]

    def pair_blocks(self, out, atom_scale):
        return zip(out, [None] * len(out) if atom_scale is None else self.atoms_out(atom_scale))

    def displacement(self):
        total = self.atom_off[-1]
        names = "(S, 3) or (q, S, 3)" if self.dim == 3 else "(S,) or (q, S)"
        return (), ((total, 3) if self.dim == 3 else (total,)), f"{names} with S = sum(sizes) = {total}"


_DEV, _PLAN = ("ctx", "w", "v", "m", "nvec", "batch"), ("plan", "w", "v", "nvec")
# consumer -> (C entry of a uniform batch, its argument prefix, C entry of a plan's slots, its argument prefix):
# _BatchSolver._call fills the prefix from the solver and appends the consumer's own arguments
_CONSUMER_ENTRIES = {
    "msf": ("sc_dev_modes_msf_f64", _DEV + ("dim",), "sc_batch_plan_modes_msf_f64", _PLAN),
    "dcc": ("sc_dev_modes_dcc_f64", _DEV + ("dim",), "sc_batch_plan_modes_dcc_f64", _PLAN),
    "aniso": ("sc_dev_modes_aniso_f64", _DEV, "sc_batch_plan_modes_aniso_f64", _PLAN),
    "distfluct": ("sc_dev_modes_distfluct_f64", _DEV, "sc_batch_plan_modes_distfluct_f64", _PLAN),
    "overlap": ("sc_dev_modes_overlap_f64", ("ctx", "v", "m", "nvec", "batch", "dim"),
                "sc_batch_plan_modes_overlap_f64", ("plan", "v", "nvec", "first_row")),
}
# the same for the consumers that return displacement fields (csrc/mode_response.hip): their C entries are named
# sc_dev_mode_* / sc_batch_plan_mode_*
_FIELD_ENTRIES = {
    "response": ("sc_dev_mode_response_f64", _DEV + ("dim",), "sc_batch_plan_mode_response_f64", _PLAN),
    "combine": ("sc_dev_mode_combine_f64", ("ctx", "v", "m", "nvec", "batch", "dim"),
                "sc_batch_plan_mode_combine_f64", ("plan", "v", "nvec", "first_row")),
}
# the same for perturbation-response scanning (csrc/mode_prs.hip): its C entries are named sc_dev_prs_f64 / sc_batch_plan_prs_f64
_SCAN_ENTRIES = {
    "prs": ("sc_dev_prs_f64", _DEV, "sc_batch_plan_prs_f64", _PLAN),
    # the generalized correlation (csrc/mode_lmi.hip)
    "lmi": ("sc_dev_lmi_f64", _DEV, "sc_batch_plan_lmi_f64", _PLAN),
}


class _BatchSolver:
    """
    What :class:`DeviceBatchSolver` and :class:`RaggedBatchSolver` share, the consumers of the solved modes included.  A
    subclass sets ``_first_row`` (global mode index of row 0 of ``w`` / ``v``), ``_common_modes`` (modes every member has: an
    explicit ``mode_subset`` is checked against them), ``_layout`` (where results lie and how they are handed back:
    :class:`_Layout`) and, for the plan's C entries, ``_plan``; it implements ``assemble`` and ``eigh``.
    """

    #: bytes the packed GEMM operands of :meth:`dcc` may take at a time (None: SPRINGCRAFT_MODES_BUDGET_BYTES, else 1 GiB)
    consumer_budget_bytes = None
    _plan = None

    def _allocate(self, m, nvec, want_vectors):
        """The tensors of a solve: ``counts`` (behind a window), ``matrix`` (batch, m, m), ``w`` (batch, nvec), ``v`` (batch, nvec, m)."""
        torch, f64 = self.torch, self.torch.float64
        self.counts = torch.zeros((self.batch,), dtype=torch.int64, device=self.device) if self.window is not None else None
        self.matrix = torch.empty((self.batch, m, m), dtype=f64, device=self.device)
        self.w = torch.empty((self.batch, nvec), dtype=f64, device=self.device)
        self.v = torch.empty((self.batch, nvec, m), dtype=f64, device=self.device) if want_vectors else None

    def set_profiling(self, on):
        self.ctx.check(self._L.sc_ctx_set_profiling(self.ctx.handle, 1 if on else 0))

    def last_timings(self):
        return _last_timings(self.ctx, self._L)

    def solve(self, coord):
        """
        One pass of the hot path over the batch: assembly + eigensolve, all on device.  Only ENQUEUES (the result tensors
        are valid in stream order); call :meth:`finish` before trusting them on the host.
        """
        self.assemble(coord)
        return self.eigh()

    def finish(self):
        """
        Wait for the solves enqueued so far and raise what they could only find out on the device:
        ``np.linalg.LinAlgError`` -- what ``np.linalg.eigh`` raises at nma.py:61 -- if a matrix held a NaN / Inf entry
        (its eigenvalues come back NaN, the other structures of the batch are unaffected) or a tridiagonal QL iteration
        did not converge.  The condition is reported once.  With ``subset_by_value``, then ValueError naming every structure
        whose window held more than ``max_modes`` eigenpairs.  Returns (w, v).
        """
        self.ctx.synchronize()
        if self.window is not None:
            counts = self.counts.cpu().numpy()
            over = np.nonzero(counts > self.max_modes)[0]
            if len(over):
                which = ", ".join(f"{b} ({counts[b]})" for b in over)
                raise ValueError(f"the eigenvalue window {self.window} holds more than max_modes = {self.max_modes} "
                                 f"eigenpairs for structure(s) {which}; their slots hold the {self.max_modes} lowest")
        return self.w, self.v

    @property
    def _ntriv(self):
        return 6 if self.dim == 3 else 1

    def _need_vectors(self):
        if self.v is None:
            raise ValueError("the mode consumers need the eigenvectors: build the solver with want_vectors=True")

    def _selection(self, mode_subset, pinv_default):
        """(ModeSelection, counts pointer) for a consumer call; every check is on the host."""
        self._need_vectors()
        rows = batch_mode_rows(mode_subset, self._ntriv, self.subset, self._common_modes, self.window)
        sel = _hip.ModeSelection()
        # (how the sc_batch_plan_modes_* entries learn the global index of row 0; the sc_dev_modes_* entries never read it)
        sel.reserved = self._first_row
        nvec = self.w.shape[1]
        keep = None
        if self.window is not None:
            sel.kind, sel.row0 = _hip.SC_SEL_FROM_ROW, 0
        elif mode_subset is None and pinv_default and self.subset is None:
            sel.kind, sel.rcond = _hip.SC_SEL_PINV, 1e-6
        elif mode_subset is None:
            # every solved non-trivial row (a ragged full-spectrum solver: the records end the rows at dim * n_b)
            sel.kind, sel.row0 = _hip.SC_SEL_FROM_ROW, _trivial_rows(self._ntriv, self._first_row, nvec)
        else:
            # through page-locked memory: a copy from pageable memory would make the host wait for the stream
            host = self.torch.from_numpy(rows).pin_memory()
            keep = host.to(self.device, non_blocking=True)
            sel.kind, sel.d_rows, sel.n_rows = _hip.SC_SEL_ROWS, keep.data_ptr(), len(rows)
        self._rows_keep = keep      # (the device list outlives the enqueued call)
        return sel, (C.c_void_p(self.counts.data_ptr()) if self.window is not None else None)

    def _device_f64(self, t, shape, name):
        """A consumer's extra input, checked on the host: a contiguous CUDA float64 tensor of ``shape`` on the solver's device."""
        torch = self.torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous CUDA float64 tensor of shape {shape}")
        if t.device != torch.device(self.device):
            raise ValueError(f"{name} is on {t.device}, the solver on {self.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"Expected {name} of shape {tuple(shape)}, got {tuple(t.shape)}")
        return C.c_void_p(t.data_ptr())

    def _vectors_in(self, t, what):
        """
        (q, single) of one or q displacement-shaped vectors per structure (``what``: "displacement" / "force"), checked
        on the host: a contiguous CUDA float64 tensor on the solver's device with one of the layout's two shapes.
        """
        torch = self.torch
        names = self._layout.displacement()[2]
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous CUDA float64 tensor of shape {names}")
        if t.device != torch.device(self.device):
            raise ValueError(f"{what} is on {t.device}, the solver on {self.device}")
        return self._layout.displacement_q(t.shape, what)

    def _empty(self, shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.device)

    def _call(self, consumer, *args):
        """Enqueues ``consumer``'s C entry for this solver's layout: the entry's argument prefix, then ``args``."""
        row = next(t[consumer] for t in (_CONSUMER_ENTRIES, _FIELD_ENTRIES, _SCAN_ENTRIES) if consumer in t)
        entry, prefix = row[2:] if self._layout.ragged else row[:2]
        have = {"ctx": self.ctx.handle, "plan": self._plan, "w": C.c_void_p(self.w.data_ptr()),
                "v": C.c_void_p(self.v.data_ptr()), "m": self.v.shape[2], "nvec": self.w.shape[1], "batch": self.batch,
                "dim": self.dim, "first_row": self._first_row}
        self.ctx.check(getattr(self._L, entry)(*[have[k] for k in prefix], *args))

    # ---- consumers of the solved modes (reference: nma.py:66-359, there for one model) --------------------------------
    # One body each for both solvers: self._layout says where the results lie, _CONSUMER_ENTRIES / _FIELD_ENTRIES which C entry runs.  Like
    # solve() they ONLY ENQUEUE on the solver's stream and return CUDA tensors that are valid in stream order: no
    # synchronisation, no host copy of w.  The one exception is the first call of a kind, which allocates its workspace.
    # The docstrings give the result of a DeviceBatchSolver first; a RaggedBatchSolver returns, per structure, a list of
    # views into one packed buffer (see its class docstring for the packing), with n_atoms the structure's own n_i.

    def frequencies(self):
        """
        (batch, nvec) frequencies ``sqrt(lambda) / (2 pi)`` of the solved modes; rows whose global mode index is trivial
        enter as ``abs(lambda)`` (nma.py:66-105).  With ``subset_by_value`` the mode indices are not known, so no row is
        treated as trivial (a negative rounding-level eigenvalue gives NaN, as do the padding rows).
        Ragged: [(rows_i,), ...], (dim n_i,) for a full-spectrum solver, else all ``nvec`` rows (with ``subset_by_value``
        the rows behind the count are NaN).
        """
        w = self.w.clone()
        if self.window is None:
            k = _trivial_rows(self._ntriv, self._first_row, w.shape[1])
            w[:, :k] = w[:, :k].abs()
        return self._layout.rows_out(self.torch.sqrt(w) / (2 * np.pi))

    def _per_atom(self, consumer, tail, mode_subset, tem, tem_factors):
        """The packed per-atom buffer of ``consumer`` ("msf" / "aniso": ``tail`` values per atom), ``tem`` applied."""
        sel, counts = self._selection(mode_subset, pinv_default=False)
        out = self._empty(self._layout.atoms_shape(tail))
        self._call(consumer, C.byref(sel), counts, C.c_void_p(out.data_ptr()))
        if tem is not None:
            out *= tem * tem_factors
        return out

    def mean_square_fluctuation(self, mode_subset=None, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms) mean square fluctuations ``sum_k v_k^2 / lambda_k`` over the selected modes (nma.py:108-184), one
        pass over the selected rows of ``v`` on the device.  Ragged: [(n_i,), ...].

        ``mode_subset`` holds GLOBAL ascending mode indices as in the reference, never row numbers of ``v``
        (:func:`batch_mode_rows`); None takes every solved mode that is not trivial (ragged: every own non-trivial solved
        mode of each structure; an explicit ``mode_subset`` holds global mode indices below ``dim * min(sizes)``).  With
        ``subset_by_value`` it must be None and the selection is the window: the first ``min(counts[b], max_modes)`` rows
        of structure b, read from ``counts`` on the device; a structure with an empty window gives zeros.  Whether the
        window contains trivial modes is the caller's choice of ``vl``: an ANM's six trivial eigenvalues are ~0 at rounding
        level, of either sign, so ``vl = -inf`` includes them and a small positive ``vl`` (e.g. 1e-6 lambda_max) leaves
        them out.
        A structure whose solve failed (NaN eigenvalues) gives NaN, its neighbours are unaffected; behind a window solve such
        a structure has count 0 and gives the empty window's result.
        """
        return self._layout.atoms_out(self._per_atom("msf", (), mode_subset, tem, tem_factors))

    def bfactor(self, mode_subset=None, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms) isotropic B-factors, ``8 pi^2 / 3`` times :meth:`mean_square_fluctuation` (nma.py:187-230).
        Ragged: [(n_i,), ...].
        """
        out = self._per_atom("msf", (), mode_subset, tem, tem_factors)
        out *= (8 * np.pi**2) / 3
        return self._layout.atoms_out(out)

    def _aniso_packed(self, mode_subset=None, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms, 6): every tensor's six distinct entries xx yy zz xy xz yz, as the kernel leaves them.  Ragged:
        (sum(sizes), 6), the structures back to back.
        """
        if self.dim != 3:
            raise ValueError("anisotropic fluctuation tensors need an ANM solver (dim=3)")
        return self._per_atom("aniso", (6,), mode_subset, tem, tem_factors)

    def anisotropic_fluctuation(self, mode_subset=None, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms, 3, 3) anisotropic fluctuation tensors ``sum_k v_k[a] v_k[a]^T / lambda_k`` over the selected
        modes (:func:`nma.anisotropic_fluctuation`): symmetric, and their traces are :meth:`mean_square_fluctuation` of
        the same selection, whose ``mode_subset``, window and failed-structure rules apply unchanged.  One pass over the
        selected rows of ``v``; ANM solvers only (``dim != 3`` raises ValueError before anything is enqueued).
        Ragged: [(n_i, 3, 3), ...], views into one packed tensor.
        """
        return self._layout.atoms_out(_aniso_expand(self, self._aniso_packed(mode_subset, tem, tem_factors)))

    def _overlap_call(self, d, q, want_collectivity):
        nvec = self.w.shape[1]
        ov = self._empty((self.batch, q, nvec)) if q else None
        co = self._empty((self.batch, nvec)) if want_collectivity else None
        if ov is not None or co is not None:
            self._call("overlap", C.c_void_p(d.data_ptr()) if q else None, q,
                       C.c_void_p(self.counts.data_ptr()) if self.window is not None else None,
                       C.c_void_p(ov.data_ptr()) if q else None, C.c_void_p(co.data_ptr()) if want_collectivity else None)
            # a structure whose solve failed is solved as the zero matrix: its eigenvalues are NaN, its rows of v some
            # finite basis without a meaning.  The kernel does not read w, so a row is NaN here where its eigenvalue is
            # (also the rows behind a window's count, which the kernel has set already); enqueued, like the kernel
            bad = self.torch.isnan(self.w)
            if ov is not None:
                ov.masked_fill_(bad[:, None, :], float("nan"))
            if co is not None:
                co.masked_fill_(bad, float("nan"))
        return ov, co

    def overlap(self, displacement):
        """
        Overlaps ``<v_r, d> / (|v_r| |d|)`` of every row of ``v`` with the structure's displacement(s): which modes carry
        an observed change (:func:`nma.overlap`; no reference counterpart).  ``displacement`` is a contiguous CUDA float64
        tensor (batch, n_atoms, 3) or (batch, q, n_atoms, 3) -- for a GNM solver (batch, n_atoms) or (batch, q, n_atoms)
        -- in the coordinates of the modes: with ``masses`` pass ``sqrt(mass) * d``, it is not done for you.  Returns
        (batch, nvec) / (batch, q, nvec), signed, for ALL rows of ``w`` / ``v``, trivial ones included: slice as needed.
        A row is NaN where its eigenvalue in ``w`` is: behind a window's count, and everywhere in a structure whose solve
        failed (its ``v`` holds a finite basis without a meaning); a zero displacement gives NaN too.
        One pass along the rows of ``v``; only enqueues on the solver's stream.
        Ragged: ``displacement`` is packed like the coordinates :meth:`solve` takes, (sum(sizes), 3) or (q, sum(sizes), 3)
        -- for a GNM solver (sum(sizes),) or (q, sum(sizes)) -- structure i's atoms at ``offsets[i]``; returns
        [(rows_i,), ...] or [(q, rows_i), ...], the views cut as :meth:`frequencies` cuts them ((dim n_i,) on a
        full-spectrum solver, else all ``nvec`` rows, NaN behind a window's count); only a structure's own columns are read.
        """
        self._need_vectors()
        d = displacement
        q, single = self._vectors_in(d, "displacement")
        ov = self._empty((self.batch, 0, self.w.shape[1])) if q == 0 else self._overlap_call(d, q, False)[0]
        return self._layout.rows_out(ov, single)

    def collectivity(self):
        """
        (batch, nvec) collectivities ``exp(-sum_a p_a ln p_a) / n_atoms`` of every row of ``v`` (:func:`nma.collectivity`;
        no reference counterpart): 1 for a rigid translation, 1 / n_atoms for a mode on one atom.  All rows, NaN behind a
        window's count.  Only enqueues.  Ragged: [(rows_i,), ...], cut as :meth:`frequencies` cuts them; n_atoms is the
        structure's own size.
        """
        self._need_vectors()
        return self._layout.rows_out(self._overlap_call(None, 0, True)[1])

    def distance_fluctuation(self, coord, mode_subset=None, projected=True, atom_scale=None, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms, n_atoms) fluctuations of the inter-atom distances over the selected modes
        (:func:`nma.distance_fluctuation`; no reference counterpart, ProDy: ``calcDistFlucts`` / ``calcMechStiff``):
        ``F[b, a, c] = sum_k (n_ac . (u_k[c] - u_k[a]))^2 / lambda_k`` with ``n_ac`` the unit vector from atom a to atom c
        of ``coord``, the (batch, n_atoms, 3) CUDA float64 tensor given to :meth:`solve`.  :func:`nma.effective_stiffness`
        turns it into the distances' harmonic constants on the device.

        ``mode_subset``, the window, ``subset_by_index`` and failed structures exactly as in
        :meth:`mean_square_fluctuation`.  ``atom_scale``: None, or a (batch, n_atoms) CUDA float64 tensor with ``u_k[a] =
        atom_scale[a] * v_k[a]``; None takes the rows of ``v`` as they are, like every other consumer, so a solver with
        ``masses`` wants ``atom_scale=solver.inv_sqrt_mass`` for Cartesian distances.
        ``projected=True`` (ANM solvers; ``dim != 3`` raises ValueError before anything is enqueued) sums every pair
        directly on the device: ``F`` equals its transpose bit for bit, the diagonal is exactly 0 (also in a failed
        structure, whose other entries are NaN), two distinct atoms at one position give NaN for that pair, and a
        structure's bits do not depend on the batch size or its position.  ``projected=False`` is ``c_aa + c_cc - 2
        c_ac`` of ``dcc(norm=False)`` over the same selection (GNM and ANM; ``coord`` is only checked).
        Only enqueues.
        Ragged: [(n_i, n_i), ...], views into one buffer packed like :meth:`dcc`'s.  ``coord`` is the packed (sum(sizes), 3)
        tensor given to :meth:`solve`, ``atom_scale`` None or a packed (sum(sizes),) tensor.  Every structure is summed
        over its own atoms and rows: pad rows never carry a weight, pad columns are never read.
        """
        lay = self._layout
        if projected and self.dim != 3:
            raise ValueError("projected distance fluctuations need an ANM solver (dim=3); use projected=False")
        self._need_vectors()
        cp = self._device_f64(coord, lay.atoms_shape((3,)), "coord")
        sp = None if atom_scale is None else self._device_f64(atom_scale, lay.atoms_shape(), "atom_scale")
        sel, counts = self._selection(mode_subset, pinv_default=False)
        buf = self._empty(lay.pairs_shape())
        out = lay.pairs_out(buf)
        if projected:
            self._call("distfluct", C.byref(sel), counts, cp, sp, C.c_void_p(buf.data_ptr()))
        else:
            self._call("dcc", C.byref(sel), counts, 0, int(self.consumer_budget_bytes or 0), C.c_void_p(buf.data_ptr()))
            # in place, so that a ragged result stays views of one buffer; (-2 c) + (d_a + d_c) has the bits of
            # (d_a + d_c) - 2 c: the doubling is exact and IEEE addition commutes
            for c, scale in lay.pair_blocks(out, atom_scale):
                if scale is not None:
                    c *= scale[..., :, None] * scale[..., None, :]
                diag = c.diagonal(dim1=-2, dim2=-1).clone()
                c *= -2
                c += diag[..., :, None] + diag[..., None, :]
        if tem is not None:
            buf *= tem * tem_factors
        return out

    def linear_response(self, force, mode_subset=None, atom_scale=None):
        """
        (batch, n_atoms, 3) displacements ``sum_k v_k <v_k, f> / lambda_k`` over the selected modes in answer to the
        structure's force(s) (nma.py:422-473, there ``covariance @ force`` for one model): computed in mode space, one
        pass along and one across the selected rows of ``v`` per four forces, without a covariance.  ``force`` is a
        contiguous CUDA float64 tensor (batch, n_atoms, 3) or (batch, q, n_atoms, 3); the result has its shape.  ANM solvers
        only (``dim != 3`` raises ValueError before anything is enqueued).

        ``mode_subset``, the window, ``subset_by_index`` and failed structures (NaN) exactly as in
        :meth:`mean_square_fluctuation`, except that None on a full-spectrum solver takes the reference's covariance rule
        as :meth:`dcc` does: every mode with ``|lambda| > 1e-6 max|lambda|`` of that structure -- the result is
        ``pinv(H, rcond=1e-6) @ f``.  ``atom_scale``: None, or a (batch, n_atoms) CUDA float64 tensor ``s`` for
        ``s_a sum_k v_k[a] <v_k, s f> / lambda_k``; with ``masses``, ``atom_scale=solver.inv_sqrt_mass`` gives the Cartesian
        response ``M^-1/2 pinv(H_mw) M^-1/2 f`` (None: the modes as they are, the reference's ``covariance @ force``).
        A structure's bits do not depend on the batch size, its position, its neighbours or q.  Only enqueues.
        Ragged: ``force`` is packed like the coordinates :meth:`solve` takes, (sum(sizes), 3) or (q, sum(sizes), 3), and
        ``atom_scale`` (sum(sizes),); returns [(n_i, 3), ...] or [(q, n_i, 3), ...], views into one packed buffer.
        """
        lay = self._layout
        if self.dim != 3:
            raise ValueError("linear_response needs an ANM solver (dim=3): the reference defines it for an ANM only")
        self._need_vectors()
        q, single = self._vectors_in(force, "force")
        sp = None if atom_scale is None else self._device_f64(atom_scale, lay.atoms_shape(), "atom_scale")
        sel, counts = self._selection(mode_subset, pinv_default=True)
        buf = self._empty(lay.vectors_shape(q))
        if q:
            self._call("response", C.byref(sel), counts, C.c_void_p(force.data_ptr()), q, sp, C.c_void_p(buf.data_ptr()))
        return lay.vectors_out(buf, single)

    def _failed_structures(self):
        """(batch,) bool tensor: ``w`` holds a NaN before the structure's row limit (its solve failed).  Enqueue only."""
        torch, lay = self.torch, self._layout
        nvec = self.w.shape[1]
        lim = None
        if lay.ragged:
            if getattr(self, "_row_limits_dev", None) is None:
                host = torch.tensor(lay.row_limits, dtype=torch.int64).pin_memory()
                self._row_limits_dev = host.to(self.device, non_blocking=True)
            lim = self._row_limits_dev
        if self.window is not None:
            c = self.counts.clamp(max=nvec)
            lim = c if lim is None else torch.minimum(lim, c)
        bad = torch.isnan(self.w)
        if lim is not None:
            bad = bad & (torch.arange(nvec, device=self.device)[None, :] < lim[:, None])
        return bad.any(dim=1)

    def mode_displacement(self, coefficients, atom_scale=None):
        """
        (batch, n_atoms, 3) displacements ``sum_r c_r v_r`` built from the rows of ``v`` with the caller's coefficients
        (:func:`nma.mode_displacement`; no reference counterpart, ProDy: ``deformAtoms`` / ``traverseMode`` /
        ``sampleModes``) -- for a GNM solver (batch, n_atoms).  ``coefficients`` is a contiguous CUDA float64 tensor
        (batch, nvec) or (batch, q, nvec), the shape :meth:`overlap` returns, one coefficient per row of ``w`` / ``v``,
        trivial rows included (give them 0); the result is (batch, [q,] n_atoms, 3).  ``|d| * overlap(d)`` over a
        full spectrum gives ``d`` back.  Rows behind a window's count (and a ragged slot's pad rows) are never read,
        whatever their coefficients hold.  ``atom_scale`` as in :meth:`linear_response`: the result is ``s_a`` times the
        sum (with ``masses``, ``solver.inv_sqrt_mass`` turns mass-weighted modes into Cartesian displacements).
        A structure whose solve failed (NaN eigenvalues before its row limit; its ``v`` is a finite basis without a
        meaning) gives NaN.  One pass across the rows of ``v`` per four coefficient vectors; only enqueues.
        Ragged: ``coefficients`` is (batch, nvec) or (batch, q, nvec) all the same -- of structure i the first rows_i
        count, as :meth:`frequencies` cuts them -- and the result [(n_i, 3), ...] or [(q, n_i, 3), ...], views into one
        packed buffer; ``atom_scale`` (sum(sizes),).
        """
        lay = self._layout
        self._need_vectors()
        torch, c = self.torch, coefficients
        nvec = self.w.shape[1]
        names = f"(batch, nvec) or (batch, q, nvec) with batch = {self.batch}, nvec = {nvec}"
        if not isinstance(c, torch.Tensor) or not c.is_cuda or c.dtype != torch.float64 or not c.is_contiguous():
            raise ValueError(f"coefficients must be a contiguous CUDA float64 tensor of shape {names}")
        if c.device != torch.device(self.device):
            raise ValueError(f"coefficients is on {c.device}, the solver on {self.device}")
        shape = tuple(c.shape)
        if shape == (self.batch, nvec):
            q, single = 1, True
        elif len(shape) == 3 and shape[0] == self.batch and shape[2] == nvec:
            q, single = shape[1], False
        else:
            raise ValueError(f"Expected coefficients of shape {names}, got {shape}")
        sp = None if atom_scale is None else self._device_f64(atom_scale, lay.atoms_shape(), "atom_scale")
        buf = self._empty(lay.vectors_shape(q))
        if q:
            self._call("combine", C.c_void_p(c.data_ptr()), q,
                       C.c_void_p(self.counts.data_ptr()) if self.window is not None else None, sp,
                       C.c_void_p(buf.data_ptr()))
            # the kernel does not read w: a failed structure is masked here, enqueued like the kernel (see _overlap_call)
            bad = self._failed_structures()
            if lay.ragged:
                if getattr(self, "_sizes_dev", None) is None:
                    host = torch.tensor(lay.sizes, dtype=torch.int64).pin_memory()
                    self._sizes_dev = host.to(self.device, non_blocking=True)
                per_atom = torch.repeat_interleave(bad, self._sizes_dev, output_size=lay.atom_off[-1])
                buf.masked_fill_(per_atom.view((1, -1) + (1,) * (buf.ndim - 2)), float("nan"))
            else:
                buf.masked_fill_(bad.view((-1,) + (1,) * (buf.ndim - 1)), float("nan"))
        return lay.vectors_out(buf, single)

    def dcc(self, mode_subset=None, norm=True, tem=None, tem_factors=K_B):
        """
        (batch, n_atoms, n_atoms) dynamic cross-correlations over the selected modes (nma.py:233-359); ``norm`` divides by
        ``sqrt(c_aa c_bb)``, ``tem`` is applied after the normalisation as the reference does (nma.py:355-357).
        Ragged: [(n_i, n_i), ...].

        ``mode_subset`` as in :meth:`mean_square_fluctuation`.  None on a full-spectrum solver takes, per structure, every
        mode with ``|lambda| > 1e-6 max|lambda|`` of THAT structure -- the reference's covariance rule, see :func:`nma.dcc`
        -- with the maximum found on the device (ragged: taken over the structure's OWN eigenvalues; the slot's pads are
        larger and never enter).  None on a ``subset_by_index`` solver takes every solved mode that is not
        trivial: the covariance rule needs ``lambda_max``, which such a solve does not compute.  With ``subset_by_value``
        the selection is the window (see :meth:`mean_square_fluctuation`, also for trivial modes inside it); an empty
        window gives zeros, and NaN under ``norm=True`` as 0 / 0 does in NumPy.
        """
        return self._layout.pairs_out(self._dcc_packed(mode_subset, norm, tem, tem_factors))

    def _dcc_packed(self, mode_subset, norm, tem=None, tem_factors=K_B):
        """:meth:`dcc`'s result as the one packed buffer the kernels fill."""
        sel, counts = self._selection(mode_subset, pinv_default=True)
        buf = self._empty(self._layout.pairs_shape())
        self._call("dcc", C.byref(sel), counts, int(bool(norm)), int(self.consumer_budget_bytes or 0),
                   C.c_void_p(buf.data_ptr()))
        if tem is not None:
            buf *= tem
            buf *= tem_factors
        return buf

    def prs(self, mode_subset=None, norm=True, atom_scale=None):
        """
        (batch, n_atoms, n_atoms) perturbation-response-scanning matrices (nma.py:476-524, there ``cov**2`` of one model
        reduced over its 3 x 3 blocks): ``P[b, a, c] = sum_{d, e} C_ac[d, e]^2`` with ``C_ac = sum_k u_k[a] u_k[c]^T /
        lambda_k`` over the selected modes; ``norm`` divides row a by ``P[b, a, a]``.  One kernel on the float64 matrix
        units (``csrc/mode_prs.hip``): a block ``C_ac`` is summed and squared in registers and no covariance entry is
        written to memory.  ANM solvers only (``dim != 3`` raises the reference's ValueError before anything is enqueued).

        ``mode_subset``, the window, ``subset_by_index`` and failed structures (NaN) exactly as in :meth:`dcc`: None on a
        full-spectrum solver takes the reference's covariance rule, every mode with ``|lambda| > 1e-6 max|lambda|`` of
        that structure; an empty window gives zeros, and NaN under ``norm=True`` as 0 / 0 does in NumPy.  ``atom_scale``:
        None, or a (batch, n_atoms) CUDA float64 tensor with ``u_k[a] = atom_scale[a] * v_k[a]``; None takes the rows of
        ``v`` as they are, so a solver with ``masses`` wants ``atom_scale=solver.inv_sqrt_mass`` for the Cartesian
        covariance.  With ``norm=False`` the result equals its transpose bit for bit and every entry is >= 0; a
        structure's bits do not depend on the batch size, its position or its neighbours.  Only enqueues.
        Ragged: [(n_i, n_i), ...], views into one buffer packed like :meth:`dcc`'s; ``atom_scale`` None or a packed
        (sum(sizes),) tensor.
        """
        lay = self._layout
        if self.dim != 3:
            raise ValueError("Instance of ANM class expected.")
        self._need_vectors()
        sp = None if atom_scale is None else self._device_f64(atom_scale, lay.atoms_shape(), "atom_scale")
        sel, counts = self._selection(mode_subset, pinv_default=True)
        buf = self._empty(lay.pairs_shape())
        self._call("prs", C.byref(sel), counts, sp, int(bool(norm)), C.c_void_p(buf.data_ptr()))
        return lay.pairs_out(buf)

    def prs_effector_sensor(self, mode_subset=None, norm=True, atom_scale=None):
        """
        ``(prs, effector, sensor)``: :meth:`prs` and the means of its off-diagonal entries along every row (effector) and
        every column (sensor) (nma.py:527-569), (batch, n_atoms) each, computed with torch operations on the result and
        left on the device.  Ragged: three lists, [(n_i, n_i), ...] and [(n_i,), ...] twice.
        """
        out = self.prs(mode_subset, norm, atom_scale)
        if not self._layout.ragged:
            return (out,) + _effector_sensor(self.torch, out)
        profiles = [_effector_sensor(self.torch, p) for p in out]
        return out, [e for e, _ in profiles], [s for _, s in profiles]

    def generalized_correlation(self, mode_subset=None, information=False):
        """
        (batch, n_atoms, n_atoms) generalized correlation coefficients of Lange & Grubmueller from the linear mutual
        information (:func:`nma.generalized_correlation`; no reference counterpart, Bio3D: ``lmi``, correlationplus): how
        much atom c knows about atom a's motion whatever the directions, where :meth:`dcc` is 0 for two atoms in lockstep
        along perpendicular lines.  With ``C_ac = sum_k v_k[a] v_k[c]^T / lambda_k`` over the selected modes, ``C_aa = L_a
        L_a^T`` (Cholesky, pivoted on the diagonal) and ``M = L_a^-1 C_ac L_c^-T``: ``delta = det(I - M M^T)`` clamped to
        [0, 1], ``r = sqrt(1 - delta^(1/3))`` in [0, 1]; ``information=True`` returns the mutual information
        ``-1/2 ln(delta)`` in nats instead.  The diagonal
        blocks are :meth:`anisotropic_fluctuation`'s tensors; every other block is summed on the float64 matrix units and
        reduced to its value in registers (``csrc/mode_lmi.hip``), no covariance entry is written to memory.  ANM solvers
        only: for a GNM r is ``|dcc(norm=True)|``, and ``dim != 3`` raises ValueError before anything is enqueued.

        r and I do not change under any invertible linear map per atom, so there is no ``tem`` and no ``atom_scale``: a
        solver with ``masses`` gives the Cartesian result as it is.  ``r[a, a]`` is 1.0 and ``I[a, a]`` +inf by
        definition.  An atom whose own block cannot be whitened -- a Cholesky pivot not finite or <= 2^-40 times the
        block's diagonal entry: fewer than three selected modes, an atom at rest in the selection -- has NaN in its row and
        column, diagonal included.  With exactly three selected modes every pair is perfectly correlated: r = 1 up to
        rounding, I large or +inf, never NaN.

        ``mode_subset``, the window, ``subset_by_index`` and failed structures (NaN) exactly as in :meth:`dcc`: None on a
        full-spectrum solver takes the covariance rule, every mode with ``|lambda| > 1e-6 max|lambda|`` of that structure;
        an empty selection or window gives NaN for that structure and no other.  The result equals its transpose bit for
        bit, and a structure's bits do not depend on the batch size, its position or its neighbours.  Only enqueues.
        Ragged: [(n_i, n_i), ...], views into one buffer packed like :meth:`dcc`'s; a member's bits are those of its
        uniform solve, whatever the other members and the slot order.
        """
        return self._layout.pairs_out(self._lmi_packed(mode_subset, information))

    def _lmi_packed(self, mode_subset, information):
        """:meth:`generalized_correlation`'s result as the one packed buffer the kernel fills."""
        if self.dim != 3:
            raise ValueError("generalized_correlation needs an ANM solver (dim=3): for a GNM it is abs(dcc(norm=True))")
        self._need_vectors()
        sel, counts = self._selection(mode_subset, pinv_default=True)
        buf = self._empty(self._layout.pairs_shape())
        self._call("lmi", C.byref(sel), counts, int(bool(information)), C.c_void_p(buf.data_ptr()))
        return buf

    def correlation_network(self, kind="dcc", mode_subset=None, coord=None, contact_cutoff=None, min_correlation=0.0):
        """
        The :class:`~springcraft_amd.network.CorrelationNetwork` of every structure's coupling map, computed where the map
        is: ``kind="dcc"`` takes ``dcc(mode_subset, norm=True)``, ``kind="lmi"`` ``generalized_correlation(mode_subset)``
        (ANM solvers only: ``dim != 3`` raises its ValueError).  No reference counterpart (Bio3D: ``cna`` on ``dccm`` /
        ``lmi``; the shortest paths and betweenness of a graph library on host copies of the maps).  An edge a - c exists
        where ``|c_ac| >= min_correlation`` and, with ``coord`` -- a CUDA float64 tensor shaped like the solver's coordinates
        -- and ``contact_cutoff``, the two atoms are within the cutoff; its weight is ``-log(min(|c_ac|, 1))``.  The result
        holds ``weights``, ``distances`` and ``next_hop`` as (batch, n_atoms, n_atoms) CUDA tensors, ragged: lists of (n_i,
        n_i) views of packed buffers, and ``path`` / ``path_length`` / ``usage`` / ``betweenness`` / ``reachable``.  A failed
        structure's map is NaN, so its member is flagged: NaN distances, next hops -1.  Only enqueues.

        ValueError before anything is enqueued: ``min_correlation`` outside [0, 1], a cutoff that is not positive, a cutoff
        without coordinates or the reverse, an unknown ``kind``.
        """
        from . import network as _net

        mc, cut = _net.check_network_args(min_correlation, contact_cutoff, coord is not None)
        if kind not in ("dcc", "lmi"):
            raise ValueError(f"kind must be 'dcc' or 'lmi', got {kind!r}")
        lay = self._layout
        if coord is not None:
            self._device_f64(coord, lay.atoms_shape((3,)), "coord")
        with self.torch.cuda.device(self.device):
            buf = self._dcc_packed(mode_subset, True) if kind == "dcc" else self._lmi_packed(mode_subset, False)
            sizes = lay.sizes if lay.ragged else [lay.n_atoms] * lay.batch
            form = _net._Form(_net.check_sizes(sizes), "ragged" if lay.ragged else "uniform", False)
            xyz = None if coord is None else coord.view(-1, 3)
            return _net.network_from_packed(self.torch, self.device, self.ctx, form, buf.view(-1), xyz, cut, mc,
                                            keep=(self._rows_keep,))

    # ---- how the modes of member a compare with those of member b (csrc/mode_subspace.hip) ---------------------------------
    # No reference counterpart (Bio3D: rmsip / covsoverlap; ProDy: calcSubspaceOverlap / calcCovOverlap / calcOverlap of two
    # mode sets).  Uniform layout only; like the consumers above they only enqueue.

    def _subspace_partner(self, other):
        """The second operand set of a comparison, checked on the host: ``other`` or, for None, this solver itself."""
        if self._layout.ragged:
            raise ValueError("mode subspaces can only be compared within a uniform batch: members of different size have "
                             "no common coordinates (they need an alignment first)")
        self._need_vectors()
        if other is None or other is self:
            return self
        if not isinstance(other, _BatchSolver) or other._layout.ragged:
            raise ValueError("other must be a uniform batch solver (DeviceBatchSolver): members of different size have no "
                             "common coordinates")
        if other.dim != self.dim or other.n_atoms != self.n_atoms:
            raise ValueError(f"other holds structures of {other.n_atoms} atoms with dim = {other.dim}, this solver of "
                             f"{self.n_atoms} atoms with dim = {self.dim}: their modes have no common coordinates")
        if self.torch.device(other.device) != self.torch.device(self.device):
            raise ValueError(f"other is on {other.device}, this solver on {self.device}")
        if getattr(other, "_stream", None) != getattr(self, "_stream", None):
            raise ValueError("other was built on another stream: the two solvers' contexts must enqueue on one stream")
        other._need_vectors()
        return other

    def _subspace_sets(self, other, pick):
        """
        ((sel, counts pointer) of this solver, the same of the partner or None for a self-comparison, partner); ``pick(s)``
        makes solver s's (sel, counts).  The selections' device lists are kept on their solvers.
        """
        partner = self._subspace_partner(other)
        mine = pick(self)
        return mine, (pick(partner) if partner is not self else None), partner

    def _subspace_call(self, entry, mine, theirs, partner, with_counts, *args):
        vp = C.c_void_p
        first = [vp(self.w.data_ptr()), vp(self.v.data_ptr()), C.byref(mine[0])] + ([mine[1]] if with_counts else []) + \
                [self.w.shape[1], self.batch]
        if theirs is None:
            second = [None, None, None] + ([None] if with_counts else []) + [0, 0]
        else:
            second = [vp(partner.w.data_ptr()), vp(partner.v.data_ptr()), C.byref(theirs[0])] + \
                     ([theirs[1]] if with_counts else []) + [partner.w.shape[1], partner.batch]
        self.ctx.check(getattr(self._L, entry)(self.ctx.handle, *first, *second, self.v.shape[2], *args))

    def _first_modes(self, n_modes):
        """Global indices of the first ``n_modes`` non-trivial solved modes, or of as many as were solved."""
        n_modes = int(n_modes)
        if n_modes < 0:
            raise ValueError(f"n_modes must not be negative, got {n_modes}")
        nvec = self.w.shape[1]
        r0 = _trivial_rows(self._ntriv, self._first_row, nvec)
        return self._first_row + np.arange(r0, min(r0 + n_modes, nvec))

    def rmsip(self, n_modes=10, mode_subset=None, other=None):
        """
        (batch, batch) root mean square inner products of the members' mode subspaces (Amadei 1999; Bio3D ``rmsip``, ProDy
        ``calcSubspaceOverlap``): ``RMSIP[a, b] = sqrt(sum_ij <v_a,i, v_b,j>^2 / sqrt(k_a k_b))`` over the k selected modes
        of each member -- ``sqrt(1/k sum ...)`` whenever both carry k -- 1 for equal subspaces, 0 for orthogonal ones.
        ``other``: another uniform solver of the same ``dim``, ``n_atoms``, device and stream; the result is then
        (batch, other.batch), member a of this solver against member b of ``other``, and the selection is taken on each.

        Selection: ``mode_subset`` (global mode indices as in :meth:`mean_square_fluctuation`) if given; otherwise the
        first ``n_modes`` non-trivial solved modes, or fewer if fewer were solved; behind ``subset_by_value`` the window
        itself (``n_modes`` is not read, ``mode_subset`` must be None), where the counts may differ between members and the
        formula stays defined; an empty window gives NaN, 0 / 0.  A member whose solve failed (NaN eigenvalues) turns its
        row and column into NaN and no other entry.  One kernel on the float64 matrix units (``csrc/mode_subspace.hip``):
        the inner products are accumulated, squared and summed in registers, none is written to memory.  Without ``other``
        only the pairs a >= b are computed and the result equals its transpose bit for bit; an entry's bits do not depend on
        the batch sizes, the members' positions or their neighbours.  Only enqueues.

        The rows of ``v`` are compared as they are.  There is no ``atom_scale``: the Cartesian modes of a mass-weighted
        solve are not orthonormal and an RMSIP of non-orthonormal sets is not defined without a renormalisation, which is
        out of scope; with ``masses`` this compares the mass-weighted modes.  A :class:`RaggedBatchSolver` raises
        ValueError: members of different size have no common coordinates.
        """
        return self._subspace_matrix(0, _rmsip_pick(n_modes, mode_subset), other)

    def covariance_overlap(self, mode_subset=None, other=None):
        """
        (batch, batch) covariance overlaps of the members (Hess 2002; Bio3D ``covsoverlap``, ProDy ``calcCovOverlap``):
        ``1 - sqrt(max(0, T_a + T_b - 2 S_ab) / (T_a + T_b))`` with ``T = sum_i 1 / lambda_i`` the trace of a member's
        covariance over the selected modes and ``S_ab = sum_ij <v_a,i, v_b,j>^2 / sqrt(lambda_a,i lambda_b,j)`` the trace of
        the product of the two covariances' square roots: 1 for equal covariances, 0 for orthogonal ones.  ``other`` as in
        :meth:`rmsip`: (batch, other.batch).

        Selection exactly as :meth:`dcc` / :meth:`prs`: None on a full-spectrum solver takes the covariance rule, every
        mode with ``|lambda| > 1e-6 max|lambda|`` of that member; behind ``subset_by_index`` every non-trivial solved mode;
        behind ``subset_by_value`` the window; or an explicit ``mode_subset``.  A selected mode with a negative eigenvalue
        (a window that reaches below 0) gives NaN.  Kernel, failed members, bits and ``atom_scale`` as in :meth:`rmsip`.
        Only enqueues.
        """
        return self._subspace_matrix(1, _listed_pick(mode_subset, True), other)

    def _subspace_matrix(self, kind, pick, other, raw=False):
        """
        The (batch, partner.batch) result of kind 0 (RMSIP) / 1 (covariance overlap); ``raw``: (result, S, t of this
        solver's members, t of the partner's), the sums the result is formed from (the tests gate S itself).
        """
        mine, theirs, partner = self._subspace_sets(other, pick)
        out = self._empty((self.batch, partner.batch))
        s_raw = self._empty((self.batch, partner.batch)) if raw else None
        t_a = self._empty((self.batch,)) if raw else None
        t_b = self._empty((partner.batch,)) if raw and theirs is not None else None
        self._call_keep = (mine, theirs)      # (the selections' device lists outlive the enqueued call)
        vp = C.c_void_p
        self._subspace_call("sc_dev_subspace_f64", mine, theirs, partner, True, kind, vp(out.data_ptr()),
                            vp(s_raw.data_ptr()) if raw else None, vp(t_a.data_ptr()) if raw else None,
                            vp(t_b.data_ptr()) if t_b is not None else None)
        return (out, s_raw, t_a, t_a if t_b is None else t_b) if raw else out

    def mode_overlap_matrix(self, pairs, mode_subset, other=None):
        """
        (n_pairs, k, k) raw overlaps ``G[p, i, j] = <v_a,i, v_b,j>`` of the k modes of ``mode_subset`` (global mode
        indices, required: the table has one row per listed mode) for the listed member pairs ``pairs`` = [(a, b), ...]:
        the table one matches the modes of two members with (ProDy ``calcOverlap(modesA, modesB)``).  ``other`` as in
        :meth:`rmsip`: b then counts ``other``'s members.  A pair index outside the batch raises ValueError on the host.
        The kernel of :meth:`rmsip` with a store in place of the squared sum; a failed member gives NaN.  Not available
        behind ``subset_by_value`` (the modes' indices are only known on the device).  Only enqueues.
        """
        if mode_subset is None:
            raise ValueError("mode_overlap_matrix needs an explicit mode_subset: the table has one row per listed mode")

        pick = _listed_pick(mode_subset, False)
        partner = self._subspace_partner(other)
        pr = np.asarray(pairs)
        if pr.size and (pr.dtype.kind not in "iu" or pr.ndim != 2 or pr.shape[1] != 2):
            raise ValueError("pairs must be (n_pairs, 2) integer member indices")
        pr = pr.astype(np.int64) if pr.size else np.zeros((0, 2), dtype=np.int64)
        if pr.size and (pr.min() < 0 or pr[:, 0].max() >= self.batch or pr[:, 1].max() >= partner.batch):
            raise ValueError(f"pairs must name members (a, b) with 0 <= a < {self.batch} and 0 <= b < {partner.batch}")
        mine, theirs, partner = self._subspace_sets(other, pick)
        k = int(mine[0].n_rows)
        out = self._empty((len(pr), k, k))
        if len(pr) and k:
            host = self.torch.from_numpy(np.ascontiguousarray(pr, dtype=np.int32)).pin_memory()
            dev = host.to(self.device, non_blocking=True)
            self._call_keep = (mine, theirs, dev)
            self._subspace_call("sc_dev_subspace_gram_f64", mine, theirs, partner, False, C.c_void_p(dev.data_ptr()),
                                len(pr), C.c_void_p(out.data_ptr()))
        return out


class _ReducedSolver(_BatchSolver):
    """
    What the reduced-model solvers share (:class:`RTB`, :class:`Subsystem`, :class:`SubsystemBatch`): each builds networks
    from the device's contact scan and the force field's constants, reduces them to ``self.matrix`` (batch, order, order) of a
    smaller order than ``m`` and solves that, fully or for an index range.
    """

    def _device_setup(self, device, batch, n_atoms, dim, order):
        """The device, the context on torch's current stream and the state of a solver of ``batch`` matrices of ``order``."""
        import torch

        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._L = _hip.lib()
        self._stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = _hip.Context(self.device.index, stream=self._stream)
        self.batch, self.dim, self.n_atoms, self.m, self._solve_order = batch, dim, n_atoms, dim * n_atoms, order
        self.window, self.max_modes, self.counts = None, None, None
        self.subset, self.nvec = None, order
        self._first_row, self._common_modes = 0, order
        self._layout = _UniformLayout(batch, n_atoms, dim)
        self.matrix = self.w = self.v = None
        self._plans = {}

    def _scan_network(self, coord, force_field, who=""):
        """
        ``(pairs, gamma)`` of one structure: the device scans the contacts, ``force_constant()`` gives the constants of the
        ordered pairs on the host (as ``compute_hessian`` does for a user-defined force field).  ``who`` opens the message.
        """
        from .interaction import _normalised_patch, _pair_list

        if id(force_field) not in self._plans:
            self._plans[id(force_field)] = device_plan(force_field)[:2]
        ff_desc, patch = self._plans[id(force_field)]
        keep = []
        patch_desc = _normalised_patch(patch, len(coord), keep)
        pairs, sq_dist = _pair_list(self.ctx, coord, ff_desc, patch_desc, want_sq_dist=True)
        gamma = np.ascontiguousarray(force_field.force_constant(pairs[:, 0], pairs[:, 1], sq_dist), dtype=np.float64)
        if gamma.shape != (len(pairs),):
            raise ValueError(f"{who}force_constant() returned shape {gamma.shape} for {len(pairs)} pairs")
        return pairs, gamma

    def _need_vectors(self):
        if self.v is None:
            raise ValueError("the mode consumers need the modes: call solve() first")

    def _index_subset(self, subset_by_index):
        """What ``solve(subset_by_index)`` asks for: every mode of the reduced matrix, or the modes lo..hi (inclusive)."""
        if subset_by_index is None:
            self.subset, self.nvec, self._first_row = None, self._solve_order, 0
        else:
            lo, hi = (int(x) for x in subset_by_index)
            if not 0 <= lo <= hi < self._solve_order:
                raise ValueError(f"subset_by_index {tuple(subset_by_index)} outside 0..{self._solve_order - 1}")
            self.subset, self.nvec, self._first_row = (lo, hi), hi - lo + 1, lo

    def _eigh_reduced(self, vectors):
        """Eigendecomposes ``self.matrix`` (destroyed) into ``self.w`` (batch, nvec) and ``vectors`` (batch, nvec, order)."""
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        if self.subset is None:
            self.ctx.check(self._L.sc_dev_eigh_f64(self.ctx.handle, p(self.matrix), self._solve_order, self.batch, p(self.w),
                                                   p(vectors)))
        else:
            self.ctx.check(self._L.sc_dev_eigh_range_f64(self.ctx.handle, p(self.matrix), self._solve_order, self.batch,
                                                         self.subset[0], self.subset[1], p(self.w), p(vectors)))


class DeviceBatchSolver(_BatchSolver):
    """
    ANM (dim=3) or GNM (dim=1) eigensolves for a batch of equally sized structures whose
    coordinates already live in HBM.  Buffers are torch CUDA tensors; all work is enqueued on
    torch's current stream through a ``sc_ctx`` bound to that stream.

    ``masses``: None, or (batch, n_atoms) / (n_atoms,) atomic masses: the matrices are mass-weighted as
    ``ANM.hessian`` / ``GNM.kirchhoff`` do (anm.py:89-94,112-113; gnm.py:85-87,104-105).
    ``subset_by_index=(lo, hi)``: only the eigenpairs with ascending index lo..hi (inclusive) through the
    partial-spectrum path (no reference counterpart; BASELINE config 5): ``w`` is (batch, m), ``v`` (batch, m, n).
    ``subset_by_value=(vl, vu)`` with ``max_modes=K``: the eigenpairs whose eigenvalues lie in (vl, vu] (scipy's
    semantics, see :func:`nma.eigh`), counted per structure on the device, so :meth:`solve` still only enqueues.  ``w`` is
    (batch, K), ``v`` (batch, K, n) and ``counts`` an int64 tensor (batch,) of the true counts: structure b's first
    ``min(counts[b], K)`` rows are its window in ascending order, the rest NaN (``w``) / zero (``v``).  :meth:`finish`
    raises ValueError for structures whose window held more than K eigenpairs (their slots keep the K lowest).
    Structures of different sizes, patched or tabulated force fields: :class:`RaggedBatchSolver`.

    The consumers of the solved modes (:meth:`frequencies` ... :meth:`dcc`, documented on the shared base) return one CUDA
    tensor each with a leading batch axis: (batch, n_atoms[, 3, 3]) per atom, (batch, n_atoms, n_atoms) per pair,
    (batch, [q,] nvec) per row of ``v`` and (batch, [q,] n_atoms, 3) per displacement field.
    """

    def __init__(self, n_atoms, batch, force_field, dim=3, device=None, want_vectors=True, masses=None,
                 subset_by_index=None, subset_by_value=None, max_modes=None):
        from .nma import _value_window

        m = int(n_atoms) * int(dim)
        self.window = _value_window(subset_by_value, subset_by_index)
        if self.window is None and max_modes is not None:
            raise ValueError("max_modes applies to subset_by_value only")
        if self.window is not None:
            if max_modes is None:
                raise ValueError("subset_by_value needs max_modes, the number of eigenpairs kept per structure")
            if not 1 <= int(max_modes) <= m:
                raise ValueError(f"max_modes {max_modes} outside 1..{m}")
            max_modes = int(max_modes)
        import torch

        self.torch = torch
        self.n_atoms, self.batch, self.dim = int(n_atoms), int(batch), int(dim)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        ff_desc, patch, fused = device_plan(force_field)
        if not fused or patch is not None or ff_desc.kind == _hip.SC_FF_TABULATED:
            raise ValueError("DeviceBatchSolver takes Invariant / Hinsen / ParameterFree force fields; use "
                             "RaggedBatchSolver for patched or tabulated ones")
        self._ff = ff_desc
        self._L = _hip.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = _hip.Context(self.device.index, stream=stream)
        self._stream = stream     # (two solvers are compared on one stream: _subspace_partner)
        m = self.n_atoms * self.dim
        self.m = m
        f64 = torch.float64
        self._layout = _UniformLayout(self.batch, self.n_atoms, self.dim)
        self.subset = None
        nvec = m
        if subset_by_index is not None:
            lo, hi = int(subset_by_index[0]), int(subset_by_index[1])
            if not 0 <= lo <= hi < m:
                raise ValueError(f"subset_by_index {subset_by_index} outside 0..{m - 1}")
            self.subset = (lo, hi)
            nvec = hi - lo + 1
        self._first_row, self._common_modes = (self.subset[0] if self.subset else 0), m
        self.max_modes = max_modes
        self._allocate(m, max_modes if self.window is not None else nvec, want_vectors)
        self.inv_sqrt_mass = None
        if masses is not None:
            mm = torch.as_tensor(np.asarray(masses, dtype=np.float64) if not torch.is_tensor(masses) else masses,
                                 dtype=f64, device=self.device)
            if mm.ndim == 1:
                mm = mm[None, :].expand(self.batch, -1)
            if tuple(mm.shape) != (self.batch, self.n_atoms):
                raise IndexError(f"{tuple(mm.shape)} masses for a batch of {self.batch} x {self.n_atoms} atoms")
            if bool((mm == 0).any()):
                raise ValueError("masses must not be 0")          # anm.py:85-86
            self.inv_sqrt_mass = (1.0 / torch.sqrt(mm)).contiguous()

    def assemble(self, coord):
        """coord: (batch, n_atoms, 3) float64 CUDA tensor -> self.matrix (Hessian / Kirchhoff)."""
        assert coord.is_cuda and coord.dtype == self.torch.float64 and coord.is_contiguous()
        assert tuple(coord.shape) == (self.batch, self.n_atoms, 3)
        fn = self._L.sc_dev_hessian_f64 if self.dim == 3 else self._L.sc_dev_kirchhoff_f64
        wp = C.c_void_p(self.inv_sqrt_mass.data_ptr()) if self.inv_sqrt_mass is not None else None
        self.ctx.check(fn(self.ctx.handle, C.c_void_p(coord.data_ptr()), self.n_atoms, self.batch,
                          C.byref(self._ff), wp, C.c_void_p(self.matrix.data_ptr())))
        return self.matrix

    def eigh(self):
        """Eigendecompose self.matrix (destroyed) -> (w, v) tensors; v rows are modes (nma.py:63)."""
        vp = C.c_void_p(self.v.data_ptr()) if self.v is not None else None
        if self.window is not None:
            self.ctx.check(self._L.sc_dev_eigh_window_f64(self.ctx.handle, C.c_void_p(self.matrix.data_ptr()), self.m,
                                                          self.batch, self.window[0], self.window[1], self.max_modes,
                                                          C.c_void_p(self.w.data_ptr()), vp,
                                                          C.c_void_p(self.counts.data_ptr())))
        elif self.subset is None:
            self.ctx.check(self._L.sc_dev_eigh_f64(self.ctx.handle, C.c_void_p(self.matrix.data_ptr()), self.m,
                                                   self.batch, C.c_void_p(self.w.data_ptr()), vp))
        else:
            self.ctx.check(self._L.sc_dev_eigh_range_f64(self.ctx.handle, C.c_void_p(self.matrix.data_ptr()), self.m,
                                                         self.batch, self.subset[0], self.subset[1],
                                                         C.c_void_p(self.w.data_ptr()), vp))
        return self.w, self.v


class RaggedBatchSolver(_BatchSolver):
    """
    ONE batched solve for structures that differ: in size, in force field -- any built-in one,
    :class:`TabulatedForceField` (forcefield.py:369-533) and :class:`PatchedForceField` (forcefield.py:117-261) around
    those included -- and in their masses (anm.py:89-94).  The reference models one arbitrary structure per object
    (anm.py:62-63); here every structure gets a slot of one common matrix order in a single batched eigensolve
    (``sc_batch_plan_*`` in the C ABI, which documents the exact padding of the slots).

    User-defined :class:`ForceField` subclasses (``force_constant()`` in Python: doc/advanced.rst:23-70,
    tests/test_interaction.py:92-116) are batched too: as soon as one member needs the host callback, the pair lists of
    ALL structures come back from one device launch (``sc_batch_plan_pairs``), every structure's force field evaluates
    its constants on its own ordered pairs exactly as interaction.py:49 / :96 do, and one device pass fills all padded
    slots (``sc_batch_plan_fill_from_pairs_f64``; asymmetric constants honoured as interaction.py:50-52,103-104).

    sizes         atom counts, one per structure
    force_fields  one force field for all structures (only if it is not bound to particular atoms) or one per structure
    masses        None, or one entry per structure: None or an (n_atoms,) array
    order         common matrix order, default dim * max(sizes)

    ``solve(coord)`` takes the structures' coordinates back to back, (sum(sizes), 3) float64 on the device, and returns
    the padded result tensors (w (B, order), v (B, order, order)); ``results()`` slices them into per-structure views
    (w_i (dim n_i,), v_i (dim n_i, dim n_i), rows = modes as nma.py:63).

    A slot is ``diag(M, D)`` with every pad entry above M's spectrum, so a slot's lowest eigenpairs are the structure's
    own and the partial-spectrum path applies (:func:`ragged_subset_plan` checks the arguments on the host):

    ``subset_by_index=(lo, hi)``: ``w`` (B, hi-lo+1), ``v`` (B, hi-lo+1, order); needs ``hi < dim * min(sizes)``.
    ``subset_by_value=(vl, vu)`` with ``max_modes=K <= dim * min(sizes)``: as on :class:`DeviceBatchSolver` -- scipy's
    (vl, vu], counted on the device, :meth:`solve` only enqueues, ``counts`` an int64 device tensor, :meth:`finish` raises
    ValueError for members above K -- where ``counts[b]`` counts only the structure's own ``dim * n_b`` eigenvalues (pads
    never count, also for ``vu = +inf``) and the K rows of slot b start at ``min(il_b, dim * n_b - K)``.
    ``results()`` cuts ``v_i`` to the structure's own ``dim * n_i`` columns and, behind a window solve, both to the first
    ``min(counts[i], K)`` rows.

    :meth:`frequencies`, :meth:`mean_square_fluctuation`, :meth:`bfactor`, :meth:`dcc`, :meth:`distance_fluctuation` and
    :meth:`anisotropic_fluctuation` (and, per row instead of per atom, :meth:`overlap` and :meth:`collectivity`)
    have the meaning, defaults and trivial-mode rules of :class:`DeviceBatchSolver`'s, per structure (they are the same
    methods, documented on the shared base): they only enqueue (the first call of a kind allocates its workspace) and
    return a list of CUDA tensors, (n_i,) / (n_i, n_i) / (n_i, 3, 3) / (rows_i,), views into one packed buffer: structure
    b's atoms start at ``sum(sizes[:b])`` (``offsets[b]``), its (n_b, n_b) block at ``sum(sizes[:b] ** 2)``; per-row results
    are cut to the structure's own ``dim * n_b`` rows on a full-spectrum solver, else hold all ``nvec`` rows.  Pad rows and
    columns are never read into a result, and the ``|lambda| > 1e-6 max|lambda|`` rule of the dcc default takes its maximum
    over the structure's own eigenvalues.
    """

    def __init__(self, sizes, force_fields, dim=3, masses=None, device=None, want_vectors=True, order=None,
                 subset_by_index=None, subset_by_value=None, max_modes=None):
        self.sizes = [int(n) for n in sizes]
        self.batch, self.dim = len(self.sizes), int(dim)
        self._subset_plan = ragged_subset_plan(self.sizes, self.dim, subset_by_index, subset_by_value, max_modes)
        self.subset, self.window = self._subset_plan["subset"], self._subset_plan["window"]
        self.max_modes = self._subset_plan["max_modes"]
        # an explicit mode_subset is checked against the modes EVERY structure has: one the smallest structure lacks raises
        # the "was not solved" error instead of being dropped for that structure alone
        self._first_row, self._common_modes = self._subset_plan["first_row"], self.dim * min(self.sizes)
        import torch

        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        if not isinstance(force_fields, (list, tuple)):
            force_fields = [force_fields] * self.batch
        if len(force_fields) != self.batch:
            raise ValueError(f"{len(force_fields)} force fields for {self.batch} structures")
        self._L = _hip.lib()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = _hip.Context(self.device.index, stream=stream)
        self._keep = []          # descriptor memory must outlive sc_batch_plan_create
        descs = (_hip.StructureDesc * self.batch)()
        plans = {}
        self.force_fields = list(force_fields)
        self.host_callback = False       # True: gamma comes from force_constant() in Python for the whole batch
        for b, (n, ff) in enumerate(zip(self.sizes, force_fields)):
            if ff.natoms is not None and ff.natoms != n:
                raise ValueError(f"structure {b}: the force field was built for {ff.natoms} atoms, the structure has {n}")
            if id(ff) not in plans:
                ff_desc, patch, fused = device_plan(ff)
                if not fused:
                    self.host_callback = True
                pd = None
                if patch is not None:
                    from .interaction import _normalised_patch

                    # (negative indices, boolean masks, IndexError / self-pair ValueError as compute_* raise them)
                    pd = _normalised_patch(patch, n, self._keep)
                plans[id(ff)] = (ff_desc, pd)
                self._keep += [ff_desc, pd, ff]
            ff_desc, pd = plans[id(ff)]
            descs[b].n_atoms = n
            descs[b].ff = C.pointer(ff_desc)
            descs[b].patch = C.pointer(pd) if pd is not None else None
        h = C.c_void_p()
        self.ctx.check(self._L.sc_batch_plan_create(self.ctx.handle, self.dim, descs, self.batch,
                                                    0 if order is None else int(order), C.byref(h)))
        self._plan = h
        self.order = int(self._L.sc_batch_plan_order(h))
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self._layout = _RaggedLayout(self.sizes, self.dim, self._subset_plan["row_limits"])
        self._allocate(self.order, self._subset_plan["nvec"] or self.order, want_vectors)
        self.inv_sqrt_mass = None
        if masses is not None:
            if len(masses) != self.batch:
                raise IndexError(f"{len(masses)} mass entries for {self.batch} structures")
            packed = np.ones(int(self.offsets[-1]))
            for b, mb in enumerate(masses):
                if mb is None:
                    continue
                mb = np.asarray(mb, dtype=np.float64)
                if mb.shape != (self.sizes[b],):
                    raise IndexError(f"structure {b}: {mb.shape} masses for {self.sizes[b]} atoms")   # anm.py:81-84
                if np.any(mb == 0):
                    raise ValueError("masses must not be 0")                                            # anm.py:85-86
                packed[self.offsets[b]: self.offsets[b + 1]] = 1.0 / np.sqrt(mb)
            self.inv_sqrt_mass = torch.from_numpy(packed).to(self.device)

    def assemble(self, coord):
        """coord: (sum(sizes), 3) float64 CUDA tensor -> self.matrix, one padded slot per structure."""
        assert coord.is_cuda and coord.dtype == self.torch.float64 and coord.is_contiguous()
        assert tuple(coord.shape) == (int(self.offsets[-1]), 3)
        wp = C.c_void_p(self.inv_sqrt_mass.data_ptr()) if self.inv_sqrt_mass is not None else None
        if self.host_callback:
            return self._assemble_from_pairs(coord, wp)
        self.ctx.check(self._L.sc_batch_plan_assemble_f64(self._plan, C.c_void_p(coord.data_ptr()), wp,
                                                          C.c_void_p(self.matrix.data_ptr())))
        return self.matrix

    def pairs(self, coord, want_sq_dist=True):
        """
        Ordered pair lists of all structures from ONE device launch: [(pairs_b (k_b, 2) int64, sq_dist_b (k_b,)), ...],
        per structure what ``compute_kirchhoff`` / ``compute_hessian`` return as ``pairs`` (interaction.py:177-178).
        """
        self.torch.cuda.current_stream(self.device).synchronize()     # coord may come from torch's stream
        cp = C.c_void_p(coord.data_ptr())
        counts = np.zeros(self.batch, dtype=np.int64)
        self.ctx.check(self._L.sc_batch_plan_contacts(self._plan, cp, _hip.ptr(counts)))
        k = int(counts.sum())
        pairs = np.empty((k, 2), dtype=np.int64)
        sq = np.empty(k, dtype=np.float64) if want_sq_dist else None
        off = np.zeros(self.batch + 1, dtype=np.int64)
        self.ctx.check(self._L.sc_batch_plan_pairs(self._plan, cp, k, _hip.ptr(pairs), _hip.ptr(sq), _hip.ptr(off)))
        self._pairs_flat, self._pair_off = pairs, off
        return [(pairs[off[b]: off[b + 1]], sq[off[b]: off[b + 1]] if sq is not None else None) for b in range(self.batch)]

    def _assemble_from_pairs(self, coord, wp):
        per = self.pairs(coord, want_sq_dist=True)
        gamma = np.empty(len(self._pairs_flat), dtype=np.float64)
        for b, ((pb, sqb), ff) in enumerate(zip(per, self.force_fields)):
            g = np.asarray(ff.force_constant(pb[:, 0], pb[:, 1], sqb))   # interaction.py:49,96
            if g.shape != (len(pb),):
                raise ValueError(f"structure {b}: force_constant() returned shape {g.shape} for {len(pb)} pairs")
            gamma[self._pair_off[b]: self._pair_off[b + 1]] = g          # (Tabulated returns float32: promoted here)
        self.ctx.check(self._L.sc_batch_plan_fill_from_pairs_f64(
            self._plan, C.c_void_p(coord.data_ptr()), _hip.ptr(self._pairs_flat), _hip.ptr(self._pair_off),
            _hip.ptr(gamma), wp, C.c_void_p(self.matrix.data_ptr())))
        return self.matrix

    def eigh(self):
        vp = C.c_void_p(self.v.data_ptr()) if self.v is not None else None
        ap, wp = C.c_void_p(self.matrix.data_ptr()), C.c_void_p(self.w.data_ptr())
        if self.window is not None:
            self.ctx.check(self._L.sc_batch_plan_eigh_window_f64(self._plan, ap, self.window[0], self.window[1],
                                                                 self.max_modes, wp, vp,
                                                                 C.c_void_p(self.counts.data_ptr())))
        elif self.subset is not None:
            self.ctx.check(self._L.sc_batch_plan_eigh_range_f64(self._plan, ap, self.subset[0], self.subset[1], wp, vp))
        else:
            self.ctx.check(self._L.sc_dev_eigh_f64(self.ctx.handle, ap, self.order, self.batch, wp, vp))
        return self.w, self.v

    def results(self):
        """
        Per-structure views of the last solve: [(w_i, v_i or None), ...], ``v_i`` cut to the structure's own ``dim n_i``
        columns; behind a window solve both are cut to the first ``min(counts[i], max_modes)`` rows.  Waits for the solve
        and raises ``np.linalg.LinAlgError`` as ``np.linalg.eigh`` does at nma.py:61 (see :meth:`finish`).
        """
        self.ctx.synchronize()
        rows = list(self._subset_plan["row_limits"])
        if self.window is not None:
            rows = [min(int(c), self.max_modes) for c in self.counts.cpu().numpy()]
        out = []
        for b, n in enumerate(self.sizes):
            m = self.dim * n
            out.append((self.w[b, :rows[b]], self.v[b, :rows[b], :m] if self.v is not None else None))
        return out

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._L.sc_batch_plan_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def size_buckets(sizes, max_flop_ratio=1.25):
    """
    Groups structures whose sizes are close enough to share one padded batch: sorted by size, largest first, a bucket
    takes every structure with (N_max / N)^3 <= max_flop_ratio (the eigensolve costs ~ order^3, so no member pays more
    than that factor for its padding).  Returns lists of item indices, each in ascending item order; deterministic.
    """
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
    buckets, cur, n_max = [], [], None
    for i in order:
        if cur and (n_max / sizes[i]) ** 3 > max_flop_ratio:
            buckets.append(sorted(cur))
            cur = []
        if not cur:
            n_max = sizes[i]
        cur.append(i)
    if cur:
        buckets.append(sorted(cur))
    return buckets


def _last_timings(ctx, L):
    """Phase durations (ms) of the context's most recent profiled eigensolve as a dict."""
    t = (C.c_double * 6)()
    ctx.check(L.sc_last_eigh_timings(ctx.handle, t))
    out = {"tridiag_ms": t[0], "tridiag_eigen_ms": t[1], "backtransform_ms": t[2]}
    if t[5] > 0:   # two-stage tridiagonalisation
        out.update(two_stage=True, band_reduction_ms=t[3], bulge_chasing_ms=t[4], bt2_apply_ms=t[5])
    else:
        out.update(two_stage=False, symv_ms=t[3], syr2k_ms=t[4])
    for name in ("resident_tridiag", "panel_qr", "symm", "syr2k", "dia_tfactor", "dc_gemm", "bt1_w", "bt1_update", "sturm",
                 "stein", "cholqr"):
        ms = C.c_double(0.0)
        if L.sc_last_eigh_phase_ms(ctx.handle, name.encode(), C.byref(ms)) == 0 and name + "_ms" not in out:
            out[name + "_ms"] = ms.value
    # (not a time: 1e9 flops of the D&C merge GEMMs, summed on the device from their records -- the sizes depend on deflation)
    g = C.c_double(0.0)
    if L.sc_last_eigh_phase_ms(ctx.handle, b"dc_gemm_gflop", C.byref(g)) == 0:
        out["dc_gemm_gflop"] = g.value
    return out


def solve_sharded(coords, force_field, dim=3, want_vectors=False, group=None, solver_factory=None, solver=None):
    """
    Solve ``len(coords)`` independent structures over all ranks of ``group``.

    ``coords``: (B, n_atoms, 3) float64 ndarray on the ROOT rank (rank 0); other ranks pass None.
    Returns on rank 0 the (B, dim*n_atoms) eigenvalue array (and, if ``want_vectors``, nothing more:
    eigenvectors stay sharded on the ranks that computed them and are returned per rank); on
    other ranks returns that rank's local results.

    Exchange steps (the only communication): scatter of coordinate shards, gather of eigenvalues.
    A solve that fails on the device (NaN / Inf in a matrix, QL iteration without convergence) raises
    ``np.linalg.LinAlgError`` -- what ``np.linalg.eigh`` raises at nma.py:61 -- on the rank it happened on AND on the
    root, both after the gather (the flag travels with the eigenvalues, so no rank is left waiting in a collective).
    ``solver_factory(n_atoms, batch)`` may replace the device solver (used by the CPU/gloo tests,
    which check the sharding and the collectives, not the arithmetic).  ``solver``: a
    :class:`DeviceBatchSolver` built for this rank's shard size, reused across calls (its buffers and
    the eigensolver workspace are then allocated once).
    """
    import torch
    import torch.distributed as dist

    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if distributed else 0
    world = dist.get_world_size(group) if distributed else 1
    backend = dist.get_backend(group) if distributed else None
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" or (
        not distributed and torch.cuda.is_available()) else torch.device("cpu")

    # ---- metadata: (B, n_atoms) from the root ------------------------------------------------------
    meta = torch.zeros(2, dtype=torch.int64, device=dev)
    if rank == 0:
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        meta[0], meta[1] = coords.shape[0], coords.shape[1]
    if distributed:
        dist.broadcast(meta, src=0, group=group)
    n_items, n_atoms = int(meta[0]), int(meta[1])
    lo, hi = shard_bounds(n_items, world, rank)
    max_local = shard_bounds(n_items, world, 0)[1]

    # ---- scatter coordinates (padded to equal shard sizes: scatter needs uniform shapes) -------------
    local = torch.zeros((max_local, n_atoms, 3), dtype=torch.float64, device=dev)
    if distributed:
        chunks = None
        if rank == 0:
            full = torch.from_numpy(coords).to(dev)
            chunks = []
            for r in range(world):
                a, b = shard_bounds(n_items, world, r)
                c = torch.zeros((max_local, n_atoms, 3), dtype=torch.float64, device=dev)
                c[: b - a] = full[a:b]
                chunks.append(c)
        dist.scatter(local, chunks, src=0, group=group)
    else:
        local[: hi - lo] = torch.from_numpy(coords[lo:hi]).to(dev)

    # ---- local solve ----------------------------------------------------------------------------------
    nloc = hi - lo
    m = n_atoms * dim
    # (row max_local of the gathered buffer carries the rank's deferred solver status: 0 = fine)
    w_local = torch.zeros((max_local + 1, m), dtype=torch.float64, device=dev)
    v_local = None
    failure = None
    if nloc > 0:
        if solver_factory is None:
            if solver is None:
                solver = DeviceBatchSolver(n_atoms, nloc, force_field, dim=dim, want_vectors=want_vectors)
            elif (solver.n_atoms, solver.batch, solver.dim) != (n_atoms, nloc, dim):
                raise ValueError(f"solver was built for {(solver.n_atoms, solver.batch, solver.dim)}, "
                                 f"this rank's shard is {(n_atoms, nloc, dim)}")
            # (with a CPU backend such as gloo the shards travel as CPU tensors: onto the solver's GPU and back)
            w, v_local = solver.solve(local[:nloc].to(solver.device).contiguous())
            try:
                solver.finish()
            except np.linalg.LinAlgError as e:     # keep the collectives matched: report after the gather
                failure = e
            w_local[:nloc] = w.to(dev)
        else:
            try:
                w_np, v_local = solver_factory(n_atoms, nloc)(local[:nloc].cpu().numpy())
                w_local[:nloc] = torch.from_numpy(np.asarray(w_np)).to(dev)
            except np.linalg.LinAlgError as e:
                failure = e
                w_local[:nloc] = float("nan")
    if failure is not None:
        w_local[max_local, 0] = 1.0

    # ---- gather eigenvalues on the root -----------------------------------------------------------------
    if distributed:
        gathered = [torch.zeros_like(w_local) for _ in range(world)] if rank == 0 else None
        dist.gather(w_local, gathered, dst=0, group=group)
        if failure is not None:
            raise np.linalg.LinAlgError(f"rank {rank}: {failure}")
        if rank == 0:
            out = np.empty((n_items, m))
            failed = []
            for r in range(world):
                a, b = shard_bounds(n_items, world, r)
                g = gathered[r].cpu().numpy()
                out[a:b] = g[: b - a]
                if g[max_local, 0] != 0.0:
                    failed.append(r)
            if failed:
                raise np.linalg.LinAlgError(f"Eigenvalues did not converge on rank(s) {failed} (NaN / Inf input or a "
                                            "failed QL iteration; see that rank's exception)")
            return out, v_local
        return w_local[:nloc].cpu().numpy(), v_local
    if failure is not None:
        raise failure
    return w_local[:nloc].cpu().numpy(), v_local


def partition_lpt(costs, n_bins):
    """
    Longest-processing-time partition (structures of different sizes cost ~ N^3 each): items sorted by cost,
    largest first (ties: lower index first), each one to the currently least loaded bin (ties: lower bin).  Returns
    ``n_bins`` index lists, each in ascending item order.  Deterministic, so every rank computes the same partition
    from the broadcast sizes and no assignment has to be communicated.
    """
    costs = [float(c) for c in costs]
    order = sorted(range(len(costs)), key=lambda i: (-costs[i], i))
    load = [0.0] * n_bins
    bins = [[] for _ in range(n_bins)]
    for i in order:
        b = min(range(n_bins), key=lambda r: (load[r], r))
        bins[b].append(i)
        load[b] += costs[i]
    return [sorted(b) for b in bins]


def solve_ragged(coords_list, force_field, dim=3, group=None, solver_factory=None, solvers=None, max_flop_ratio=1.25,
                 subset_by_index=None):
    """
    Independent structures of DIFFERENT sizes over all ranks of ``group``.

    ``coords_list``: list of (N_i, 3) float64 arrays on the ROOT rank (rank 0); other ranks pass None.  The root
    broadcasts the sizes, every rank derives the same :func:`partition_lpt` with cost N_i^3, the root scatters one packed
    (padded) coordinate buffer per rank, each rank solves its structures -- ONE padded :class:`RaggedBatchSolver` batch
    per bucket of similar sizes (:func:`size_buckets`: (N_max / N)^3 <= ``max_flop_ratio``, so no member pays more than
    that factor for its padding) -- and the root gathers the packed eigenvalues.  Returns on rank 0
    the list of eigenvalue arrays in input order, on the other ranks a dict {item index: eigenvalues} of the local items.
    Two exchange steps, as in :func:`solve_sharded`; eigenvectors are not returned (they stay where they were computed,
    inside the solvers' buffers).  ``solvers``: optional dict {tuple of the bucket's sizes: RaggedBatchSolver} reused
    across calls.  Device-side failures raise ``np.linalg.LinAlgError`` after the gather, as in :func:`solve_sharded`.

    ``subset_by_index=(lo, hi)``: only eigenvalues lo..hi of every structure, through the partial-spectrum path of the
    local solvers; the result arrays are (hi-lo+1,).  Every rank checks the range against the broadcast sizes before the
    scatter (:func:`ragged_subset_plan`), so all ranks raise the same ValueError and no collective is left unmatched.  A
    ``solver_factory`` keeps its contract (full spectrum) and the columns lo..hi are sliced here.  ``solvers`` must then
    hold solvers built with the same subset.
    """
    import torch
    import torch.distributed as dist

    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if distributed else 0
    world = dist.get_world_size(group) if distributed else 1
    backend = dist.get_backend(group) if distributed else None
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" or (
        not distributed and torch.cuda.is_available() and solver_factory is None) else torch.device("cpu")

    # ---- sizes from the root ---------------------------------------------------------------------------
    n_items = torch.zeros(1, dtype=torch.int64, device=dev)
    if rank == 0:
        coords_list = [np.ascontiguousarray(c, dtype=np.float64) for c in coords_list]
        for c in coords_list:
            if c.ndim != 2 or c.shape[1] != 3:
                raise ValueError(f"every structure must be an (N, 3) coordinate array, got {c.shape}")
        n_items[0] = len(coords_list)
    if distributed:
        dist.broadcast(n_items, src=0, group=group)
    B = int(n_items[0])
    sizes = torch.zeros(max(B, 1), dtype=torch.int64, device=dev)
    if rank == 0 and B:
        sizes[:B] = torch.tensor([c.shape[0] for c in coords_list], dtype=torch.int64)
    if distributed:
        dist.broadcast(sizes, src=0, group=group)
    sizes = [int(x) for x in sizes[:B].cpu()]
    lo_col, ncol = 0, None        # columns of a structure's spectrum that travel: all, or lo .. lo + ncol - 1
    if subset_by_index is not None and B:
        lo_col, hi_col = ragged_subset_plan(sizes, dim, subset_by_index)["subset"]
        ncol = hi_col - lo_col + 1
    parts = partition_lpt([float(n) ** 3 for n in sizes], world)
    mine = parts[rank]
    atoms_per_rank = [sum(sizes[i] for i in part) for part in parts]
    pad_atoms = max(atoms_per_rank + [1])

    # ---- scatter the packed coordinates (one padded buffer per rank) -----------------------------------------
    local = torch.zeros((pad_atoms, 3), dtype=torch.float64, device=dev)
    if distributed:
        chunks = None
        if rank == 0:
            chunks = []
            for part in parts:
                c = torch.zeros((pad_atoms, 3), dtype=torch.float64, device=dev)
                off = 0
                for i in part:
                    c[off: off + sizes[i]] = torch.from_numpy(coords_list[i]).to(dev)
                    off += sizes[i]
                chunks.append(c)
        dist.scatter(local, chunks, src=0, group=group)
    else:
        off = 0
        for i in mine:
            local[off: off + sizes[i]] = torch.from_numpy(coords_list[i]).to(dev)
            off += sizes[i]

    # ---- local solves: one padded batch per bucket of similar sizes (injected CPU solvers: one per distinct size) ------
    offsets, off = {}, 0
    for i in mine:
        offsets[i] = off
        off += sizes[i]
    # (the last element of the gathered buffer carries the rank's deferred solver status: 0 = fine)
    w_local = torch.zeros(pad_atoms * dim + 1, dtype=torch.float64, device=dev)
    results = {}
    failure = None
    if solver_factory is not None:
        for n_atoms in sorted({sizes[i] for i in mine}):
            items = [i for i in mine if sizes[i] == n_atoms]
            batch = torch.stack([local[offsets[i]: offsets[i] + n_atoms] for i in items]).contiguous()
            try:
                w_np, _ = solver_factory(n_atoms, len(items))(batch.cpu().numpy())
            except np.linalg.LinAlgError as e:
                failure = e
                w_np = np.full((len(items), n_atoms * dim), np.nan)
            w = torch.from_numpy(np.asarray(w_np))
            if ncol is not None:
                w = w[:, lo_col: lo_col + ncol]
            for k, i in enumerate(items):
                w_local[offsets[i] * dim: offsets[i] * dim + w.shape[1]] = w[k].to(dev)
                results[i] = w[k].cpu().numpy().copy()
    else:
        for bucket in size_buckets([sizes[i] for i in mine], max_flop_ratio):
            items = [mine[k] for k in bucket]
            key = tuple(sizes[i] for i in items)
            solver = solvers.get(key) if solvers is not None else None
            if solver is None:
                solver = RaggedBatchSolver(key, force_field, dim=dim, want_vectors=False,
                                           subset_by_index=None if ncol is None else (lo_col, lo_col + ncol - 1))
                if solvers is not None:
                    solvers[key] = solver
            packed = torch.cat([local[offsets[i]: offsets[i] + sizes[i]] for i in items]).to(solver.device).contiguous()
            solver.solve(packed)
            try:
                per_structure = solver.results()       # waits, raises what the device found
            except np.linalg.LinAlgError as e:         # keep the collectives matched: report after the gather
                failure = e
                per_structure = solver.results()
            for i, (wi, _) in zip(items, per_structure):
                w_local[offsets[i] * dim: offsets[i] * dim + len(wi)] = wi.to(dev)
                results[i] = wi.cpu().numpy().copy()
    if failure is not None:
        w_local[-1] = 1.0

    # ---- gather the packed eigenvalues ------------------------------------------------------------------------------
    if distributed:
        gathered = [torch.zeros_like(w_local) for _ in range(world)] if rank == 0 else None
        dist.gather(w_local, gathered, dst=0, group=group)
        if failure is not None:
            raise np.linalg.LinAlgError(f"rank {rank}: {failure}")
        if rank != 0:
            return results
        out = [None] * B
        failed = []
        for r, part in enumerate(parts):
            off = 0
            buf = gathered[r].cpu().numpy()
            if buf[-1] != 0.0:
                failed.append(r)
            for i in part:
                out[i] = buf[off * dim: off * dim + (sizes[i] * dim if ncol is None else ncol)].copy()
                off += sizes[i]
        if failed:
            raise np.linalg.LinAlgError(f"Eigenvalues did not converge on rank(s) {failed} (NaN / Inf input or a failed "
                                        "QL iteration; see that rank's exception)")
        return out
    if failure is not None:
        raise failure
    return [results[i] for i in range(B)]
