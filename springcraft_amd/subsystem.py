"""
Vibrational subsystem analysis (VSA; Hinsen et al. 2000, Zheng & Brooks 2005, Ming & Wall 2005; ProDy's ``reduceModel``,
the subsystem option of Bio3D's ``nma``): how a PART of a network moves while the rest follows.  The atoms are split into a
system (s) and an environment (e); the modes of the system with the environment relaxed adiabatically are the eigenpairs of

    H_eff = H_ss - H_se H_ee^-1 H_es            (order dim n_s, the Schur complement of H_ee)

and the environment follows a system displacement as ``x_e = -H_ee^-1 H_es x_s``.  The reference has no counterpart.

:func:`subsystem_partition` validates the split on the host (NumPy only); :class:`Subsystem` assembles the three blocks on
the device straight from the pair list (``csrc/subsystem.hip``: the (dim N, dim N) matrix is never formed), reduces them with
the device Cholesky solver (``csrc/potrf.hip``), solves H_eff with the device eigensolver and hands the modes to the mode
consumers it shares with the batch solvers.
"""

import ctypes as C

import numpy as np

from . import _hip, atoms as _atoms
from .batch import _BatchSolver, _UniformLayout

__all__ = ["Subsystem", "subsystem_partition"]


def subsystem_partition(n, system):
    """
    The split of ``n`` atoms into system and environment.

    Parameters
    ----------
    n : int
    system : ndarray, shape=(n,), dtype=bool or ndarray, shape=(n_s,), dtype=int
        A mask, or the indices of the system atoms in the order the system's coordinates shall have.

    Returns
    -------
    system_index : ndarray, shape=(n_s,), dtype=int64
        As given (ascending for a mask).
    environment_index : ndarray, shape=(n_e,), dtype=int64
        Every other atom, ascending.
    group : ndarray, shape=(n,), dtype=int32
        0 for a system atom, 1 for an environment atom.
    position : ndarray, shape=(n,), dtype=int32
        The atom's place in its group.

    Raises ValueError for a mask of another length, indices that are not integers, repeat or lie outside 0..n-1, an empty
    system, and an empty environment (then there is nothing to reduce: use ANM / GNM).
    """
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be positive, got {n}")
    s = np.asarray(system)
    if s.dtype == np.bool_:
        if s.shape != (n,):
            raise ValueError(f"Expected a system mask of shape ({n},), got {s.shape}")
        idx = np.nonzero(s)[0].astype(np.int64)
    else:
        if s.ndim != 1:
            raise ValueError(f"Expected system indices of shape (n_s,), got {s.shape}")
        if len(s) and s.dtype.kind not in "iu":
            raise ValueError("system must be a boolean mask or an array of integer atom indices")
        idx = s.astype(np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"system holds an atom index outside 0..{n - 1}")
        if len(np.unique(idx)) != len(idx):
            raise ValueError("system lists an atom twice")
    if len(idx) == 0:
        raise ValueError("the system is empty")
    if len(idx) == n:
        raise ValueError("the environment is empty, there is nothing to reduce: use ANM (or GNM) on the atoms")
    group = np.ones(n, dtype=np.int32)
    group[idx] = 0
    env = np.nonzero(group)[0].astype(np.int64)
    position = np.empty(n, dtype=np.int32)
    position[idx] = np.arange(len(idx), dtype=np.int32)
    position[env] = np.arange(len(env), dtype=np.int32)
    return idx, env, group, position


class Subsystem(_BatchSolver):
    """
    Normal modes of a subsystem inside its relaxing environment, on the device.

    Parameters
    ----------
    atoms : AtomArray, shape=(n,) or ndarray, shape=(n,3), dtype=float
    force_field : ForceField, natoms=n
        Any force field, patched and tabulated ones included: the device scans the contacts, ``force_constant()`` gives the
        constants of the ordered pairs on the host, as for :class:`RTB`.  Asymmetric constants raise ValueError.
    system : ndarray, shape=(n,), dtype=bool or ndarray, shape=(n_s,), dtype=int
        The system atoms (:func:`subsystem_partition`); every other atom is environment.
    masses : bool or ndarray, shape=(n,), dtype=float, optional
        As for :class:`ANM`.  Only the SYSTEM atoms' masses are used: H_eff becomes ``T_s H_eff T_s`` with
        ``T_s = diag(1 / sqrt(m_s))``.  The environment is massless -- this is the adiabatic approximation of the method: the
        environment has no inertia and sits in its energy minimum for every position of the system.
    dim : int, optional
        3: the ANM Hessian; 1: the GNM Kirchhoff matrix.
    device : int, optional

    ``effective_hessian()`` is the (m, m) CUDA tensor H_eff, m = dim n_s, equal to its transpose bit for bit; the sums run in
    a fixed order, so two calls agree bit for bit.  ``solve(subset_by_index=None)`` enqueues assembly, reduction and eigensolve
    on torch's current stream and leaves ``w`` (1, nvec) and ``v`` (1, nvec, m), rows = unit modes of the system atoms in the
    order of ``system_index``, the dim (dim + 1) / 2 trivial modes first; ``eigen()`` returns them as host arrays.  Call
    :meth:`finish` before trusting them on the host: it raises ``np.linalg.LinAlgError`` when H_ee was not positive definite
    (an environment that can move freely), and the solver can be used again afterwards.

    After a solve every mode consumer of the batch solvers works on the system atoms, with a leading batch axis of one and
    ``n_atoms = n_s``: ``frequencies``, ``mean_square_fluctuation``, ``bfactor``, ``dcc``, ``prs``,
    ``generalized_correlation``, ``anisotropic_fluctuation``, ``overlap``, ``collectivity``, ``distance_fluctuation``,
    ``linear_response``, ``mode_displacement``, ``rmsip(other=...)``; those that need dim 3 refuse dim 1 as they always do.

    ``environment_displacement(rows=None)`` is the motion of the environment that follows the solved modes (or the q given
    rows), (nvec or q, dim n_e); ``full_modes()`` puts both together in the original atom order, (nvec, dim N).  These rows are
    NOT normalised: the system part of a row is the unit mode (in mass-weighted coordinates with ``masses``), the
    environment part is what follows it.  With H the full matrix, ``H x`` of such a row vanishes at the environment atoms and
    equals ``w_k v_k`` at the system atoms.

    ``system_index`` (n_s,), ``environment_index`` (n_e,), ``group`` and ``position`` (n,) are the host arrays of
    :func:`subsystem_partition`.
    """

    def __init__(self, atoms, force_field, system, masses=None, dim=3, device=None):
        from .forcefield import device_plan
        from .interaction import _normalised_patch, _pair_list, _validated_coord
        from .pair_operator import _checked_dim, _model_masses, check_symmetric, pair_row_start

        dim = _checked_dim(dim)
        coord = _validated_coord(_atoms.coord(atoms), force_field)
        n = len(coord)
        self.system_index, self.environment_index, self.group, self.position = subsystem_partition(n, system)
        mass = _model_masses(atoms, masses, n)
        self.masses = mass
        self.coord = coord
        self.n_total, self.n_atoms, self.n_env = n, len(self.system_index), len(self.environment_index)

        import torch

        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._L = _hip.lib()
        self._stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = _hip.Context(self.device.index, stream=self._stream)
        self.batch, self.dim, self.m, self.m_env = 1, dim, dim * self.n_atoms, dim * self.n_env
        self.window, self.max_modes, self.counts = None, None, None
        self.subset, self.nvec = None, self.m
        self._first_row, self._common_modes = 0, self.m
        self._layout = _UniformLayout(1, self.n_atoms, dim)
        self.matrix = self.w = self.v = None
        self._hes = self._hee = self._info = None
        self._reduced = False

        ff_desc, patch, _ = device_plan(force_field)
        keep = []
        patch_desc = _normalised_patch(patch, n, keep)
        pairs, sq_dist = _pair_list(self.ctx, coord, ff_desc, patch_desc, want_sq_dist=True)
        gamma = np.ascontiguousarray(force_field.force_constant(pairs[:, 0], pairs[:, 1], sq_dist), dtype=np.float64)
        if gamma.shape != (len(pairs),):
            raise ValueError(f"force_constant() returned shape {gamma.shape} for {len(pairs)} pairs")
        check_symmetric(pairs, gamma, n)
        self.n_pairs = len(pairs)
        contacts = np.bincount(pairs[:, 0], minlength=n)
        self._isolated = self.environment_index[contacts[self.environment_index] == 0]
        self._coupled = bool(np.any(self.group[pairs[:, 0]] != self.group[pairs[:, 1]]))

        with torch.cuda.device(self.device):
            dev = self.device
            self._coord = torch.from_numpy(np.array(coord)).to(dev)   # (a copy: the caller's array may be read-only)
            self._pairs = torch.from_numpy(pairs).to(dev)
            self._gamma = torch.from_numpy(gamma).to(dev)
            self._row_start = torch.from_numpy(pair_row_start(pairs, n)).to(dev)
            self._group = torch.from_numpy(self.group).to(dev)
            self._pos = torch.from_numpy(self.position).to(dev)
            self.inv_sqrt_mass = (None if mass is None else
                                  torch.from_numpy(1.0 / np.sqrt(mass[self.system_index])).to(dev)[None, :].contiguous())

    def _need_vectors(self):
        if self.v is None:
            raise ValueError("the mode consumers need the modes: call solve() first")

    def _check_network(self):
        if len(self._isolated):
            shown = ", ".join(str(a) for a in self._isolated[:10]) + (", ..." if len(self._isolated) > 10 else "")
            raise ValueError(f"{len(self._isolated)} environment atom(s) without any contact ({shown}): H_ee is singular")
        if not self._coupled:
            raise ValueError("the system shares no spring with the environment: there is nothing to reduce, and the "
                             "environment's own rigid-body motions make H_ee singular")

    # ---- assembly, reduction, eigensolve ------------------------------------------------------------------------------------
    def blocks(self):
        """``(H_ss (m, m), H_es (m_env, m), H_ee (m_env, m_env))`` as new CUDA tensors, every entry written; only enqueues."""
        out = self._empty((self.m, self.m)), self._empty((self.m_env, self.m)), self._empty((self.m_env, self.m_env))
        self._blocks_into(*out)
        return out

    def _blocks_into(self, hss, hes, hee):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self.ctx.check(self._L.sc_dev_subsystem_blocks_f64(
            self.ctx.handle, p(self._coord), self.n_total, self.dim, p(self._pairs), self.n_pairs, p(self._gamma),
            p(self._row_start), p(self._group), p(self._pos), self.n_atoms, self.n_env, p(self.inv_sqrt_mass), p(hss), p(hes),
            p(hee)))

    def _reduce_into(self, hss):
        """``hss`` <- H_eff; ``self._hee`` <- L, ``self._hes`` <- Y = L^-1 H_es, kept for the follow motion."""
        self._check_network()
        if self._hes is None:
            self._hes, self._hee = self._empty((self.m_env, self.m)), self._empty((self.m_env, self.m_env))
            self._info = self.torch.zeros((1,), dtype=self.torch.int64, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self._blocks_into(hss, self._hes, self._hee)
        self.ctx.check(self._L.sc_dev_subsystem_reduce_f64(self.ctx.handle, p(hss), p(self._hes), p(self._hee), self.m,
                                                           self.m_env, p(self._info)))
        self._reduced = True
        return hss

    def effective_hessian(self):
        """(m, m) CUDA tensor ``H_ss - H_se H_ee^-1 H_es`` (``T_s ... T_s`` with masses), every entry written; only enqueues."""
        return self._reduce_into(self._empty((self.m, self.m)))

    def _allocate(self, m, nvec, want_vectors=True):
        if self.matrix is None:
            self.matrix = self._empty((1, m, m))
        if self.w is None or self.w.shape[1] != nvec:
            self.w = self._empty((1, nvec))
            self.v = self._empty((1, nvec, m))

    def assemble(self):
        """``self.matrix`` (1, m, m) <- H_eff."""
        self._allocate(self.m, self.nvec)
        self._reduce_into(self.matrix[0])
        return self.matrix

    def eigh(self):
        """Eigendecomposes ``self.matrix`` (destroyed): (w (1, nvec), v (1, nvec, m))."""
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        if self.subset is None:
            self.ctx.check(self._L.sc_dev_eigh_f64(self.ctx.handle, p(self.matrix), self.m, 1, p(self.w), p(self.v)))
        else:
            self.ctx.check(self._L.sc_dev_eigh_range_f64(self.ctx.handle, p(self.matrix), self.m, 1, self.subset[0],
                                                         self.subset[1], p(self.w), p(self.v)))
        return self.w, self.v

    def solve(self, subset_by_index=None):
        """
        Assembly, reduction and eigensolve, all enqueued on the device: ``w`` (1, nvec), ``v`` (1, nvec, m).
        ``subset_by_index=(lo, hi)``: only the modes lo..hi (inclusive, ascending) through the partial-spectrum solver; row r
        is then mode ``lo + r``.

        An environment atom without any contact, or a system that shares no spring with the environment, makes H_ee
        singular: ValueError before anything is enqueued.  (A network of several connected parts is the caller's to avoid,
        as for an :class:`ANM`; a factorisation that fails anyway raises LinAlgError in :meth:`finish`.)
        """
        self._check_network()
        if subset_by_index is None:
            self.subset, self.nvec, self._first_row = None, self.m, 0
        else:
            lo, hi = (int(x) for x in subset_by_index)
            if not 0 <= lo <= hi < self.m:
                raise ValueError(f"subset_by_index {tuple(subset_by_index)} outside 0..{self.m - 1}")
            self.subset, self.nvec, self._first_row = (lo, hi), hi - lo + 1, lo
        self.assemble()
        return self.eigh()

    def eigen(self, subset_by_index=None):
        """
        Eigenvalues (ascending, shape (nvec,)) and modes (rows, shape (nvec, m)) of H_eff as host arrays, like
        ``ANM.eigen()``: the first dim (dim + 1) / 2 belong to rigid-body motions of the system with its environment.
        """
        self.solve(subset_by_index)
        w, v = self.finish()
        return w[0].cpu().numpy(), v[0].cpu().numpy()

    # ---- the environment's motion --------------------------------------------------------------------------------------------
    def environment_displacement(self, rows=None):
        """
        ``x_e = -H_ee^-1 H_es x_s`` for the solved modes (``rows=None``: (nvec, m_env)) or for the q rows of a contiguous
        CUDA float64 tensor (q, m) of system displacements (in mass-weighted coordinates with ``masses``).  Only enqueues.
        """
        if not self._reduced:
            raise ValueError("the follow motion needs the reduction: call solve() or effective_hessian() first")
        if rows is None:
            self._need_vectors()
            rows = self.v[0]
        else:
            q = rows.shape[0] if getattr(rows, "ndim", 0) == 2 else -1
            self._device_f64(rows, (q, self.m), "rows")
            if q < 1:
                raise ValueError(f"Expected rows of shape (q, {self.m}) with q >= 1, got {tuple(rows.shape)}")
        q = rows.shape[0]
        out = self._empty((q, self.m_env))
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self.ctx.check(self._L.sc_dev_subsystem_follow_f64(self.ctx.handle, p(self._hee), p(self._hes), self.m, self.m_env,
                                                           p(rows), q, p(out)))
        return out

    def full_modes(self):
        """
        (nvec, dim N) CUDA tensor: the solved modes at the system atoms and the follow motion at the environment atoms, in
        the original atom order.  NOT normalised (see the class docstring).
        """
        self._need_vectors()
        torch, d = self.torch, self.dim
        xe = self.environment_displacement()
        out = self._empty((self.nvec, self.n_total, d))
        out[:, torch.from_numpy(self.system_index).to(self.device)] = self.v[0].view(self.nvec, self.n_atoms, d)
        out[:, torch.from_numpy(self.environment_index).to(self.device)] = xe.view(self.nvec, self.n_env, d)
        return out.view(self.nvec, d * self.n_total)
