"""
Vibrational subsystem analysis (VSA; Hinsen et al. 2000, Zheng & Brooks 2005, Ming & Wall 2005; ProDy's ``reduceModel``,
the subsystem option of Bio3D's ``nma``): how a PART of a network moves while the rest follows.  The atoms are split into a
system (s) and an environment (e); the modes of the system with the environment relaxed adiabatically are the eigenpairs of

    H_eff = H_ss - H_se H_ee^-1 H_es            (order dim n_s, the Schur complement of H_ee)

and the environment follows a system displacement as ``x_e = -H_ee^-1 H_es x_s``.  The reference has no counterpart.

:func:`subsystem_partition` validates the split on the host (NumPy only); :class:`Subsystem` assembles the three blocks on
the device straight from the pair list (``csrc/subsystem.hip``: the (dim N, dim N) matrix is never formed), reduces them with
the device Cholesky solver (``csrc/potrf.hip``), solves H_eff with the device eigensolver and hands the modes to the mode
consumers it shares with the batch solvers.  :class:`SubsystemBatch` does that for many structures on a common core in one
batched pass and holds the one implementation of every step; a :class:`Subsystem` is its one-member case.
"""

import ctypes as C

import numpy as np

from . import _hip, atoms as _atoms
from .batch import _BatchSolver, _ReducedSolver

__all__ = ["Subsystem", "SubsystemBatch", "aligned_core", "subsystem_partition"]


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
    return _partition(n, system, False)


def _partition(n, system, allow_empty_environment):
    """:func:`subsystem_partition`; a member of a :class:`SubsystemBatch` may be exactly its system."""
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
    if len(idx) == n and not allow_empty_environment:
        raise ValueError("the environment is empty, there is nothing to reduce: use ANM (or GNM) on the atoms")
    group = np.ones(n, dtype=np.int32)
    group[idx] = 0
    env = np.nonzero(group)[0].astype(np.int64)
    position = np.empty(n, dtype=np.int32)
    position[idx] = np.arange(len(idx), dtype=np.int32)
    position[env] = np.arange(len(env), dtype=np.int32)
    return idx, env, group, position


def aligned_core(alignment):
    """
    The common core of aligned structures (NumPy only).

    Parameters
    ----------
    alignment : ndarray, shape=(B, L), dtype=int
        The atom index of member b at alignment column l, or -1 for a gap.

    Returns
    -------
    columns : ndarray, shape=(n_s,), dtype=int64
        The gap-free columns, ascending.
    systems : list of B ndarray, shape=(n_s,), dtype=int64
        Every member's atom indices at those columns: the ``systems`` of :class:`SubsystemBatch`.

    Raises ValueError for an alignment that is not a (B, L) integer array, for an index used twice within a member, for
    values below -1, and when no column is free of gaps.
    """
    a = np.asarray(alignment)
    if a.ndim != 2 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise ValueError(f"Expected an alignment of shape (B, L) with integer atom indices, got shape {a.shape}, dtype {a.dtype}")
    a = a.astype(np.int64)
    if a.size and a.min() < -1:
        raise ValueError("the alignment holds a value below -1 (-1 marks a gap, everything else is an atom index)")
    for b, row in enumerate(a):
        used = row[row >= 0]
        if len(np.unique(used)) != len(used):
            raise ValueError(f"member {b}: the alignment uses an atom index twice")
    columns = np.nonzero((a >= 0).all(axis=0))[0].astype(np.int64)
    if len(columns) == 0:
        raise ValueError("the alignment has no gap-free column: there is no common core")
    return columns, [np.ascontiguousarray(row[columns]) for row in a]


class SubsystemBatch(_ReducedSolver):
    """
    Ensemble NMA on a common core (Bio3D's ``nma.pdbs(rm.gaps=TRUE)``, ProDy's ``reduceModel`` over an ensemble): every
    member keeps ALL its atoms in its own network, each network is reduced to the aligned positions all members share by
    ``H_eff = H_ss - H_se H_ee^-1 H_es``, and the modes are compared position by position.  One batched assembly, one batched
    reduction (``csrc/subsystem.hip`` on the batched Cholesky solver) and one uniform batched eigensolve of order
    ``dim * n_s``; the result is a uniform batch solver, so every mode consumer and ``rmsip`` / ``covariance_overlap`` /
    ``mode_overlap_matrix`` run on it as on a :class:`DeviceBatchSolver`.

    Parameters
    ----------
    structures : list of B ndarray, shape=(n_b, 3), or AtomArray
        Sizes may differ.
    force_fields : ForceField or list of B ForceField
        One for all members (only if it is not bound to particular atoms) or one per member; any force field, patched and
        tabulated ones included: the device scans the contacts, ``force_constant()`` gives the constants of the ordered
        pairs on the host, as for :class:`RTB`.  Asymmetric constants raise ValueError naming the member.
    systems : list of B ndarray, shape=(n_s,), dtype=int
        The core atoms of every member, all of one length; column c of every member is the same aligned position
        (:func:`aligned_core`).  A member may be exactly its core (``n_e = 0``).
    masses : None, True, or list of B entries (None or ndarray, shape=(n_b,)), optional
        Only the core atoms' masses are used; the environment is massless, as in :class:`Subsystem`.
    dim : int, optional
    fit : bool, optional
        dim 3 only: superimpose the members first.  The cores are fitted iteratively on their running mean
        (:meth:`Ensemble.superpose`), one last fit of the original cores on the final mean gives ``(R_b, t_b)``, and every
        member's full coordinates become ``coord @ R_b.T + t_b``.  Needs ``n_s >= 3``.
    env_order : int, optional
        Atoms of an environment slot, default ``max_b n_e(b)``; a smaller value raises ValueError.  For a given
        ``env_order`` a member's ``H_eff``, ``w`` and ``v`` depend on that member alone -- not on the batch, its place in it or
        its neighbours -- but they may depend on ``env_order`` (the block plan of the factorisation does): give two batches
        the same value to compare their members bit for bit.
    device : int, optional

    ``batch = B``, ``n_atoms = n_s``, ``m = dim * n_s``, ``m_env = dim * env_order``; ``matrix`` (B, m, m), ``w`` (B, nvec),
    ``v`` (B, nvec, m), ``inv_sqrt_mass`` (B, n_s) or None.  ``fitted_coord`` (list of host arrays: the coordinates the
    networks are built from), ``core_coord`` (B, n_s, 3) CUDA tensor, and after a fit ``transforms = (R (B, 3, 3), t (B, 3))``
    and ``fit_rmsd`` (B,), host arrays (None without one).  ``system_index`` / ``environment_index`` / ``n_env`` are lists
    per member.

    :meth:`finish` raises ``np.linalg.LinAlgError`` naming the members whose H_ee was not positive definite; the other
    members' results are valid, and the solver can be used again.
    """

    _who = "member {}: "              # opens a message about member b (a Subsystem has one member and does not name it)
    _allow_empty_environment = True   # a member may be exactly its core

    def __init__(self, structures, force_fields, systems, masses=None, dim=3, fit=True, env_order=None, device=None):
        from .interaction import _validated_coord
        from .pair_operator import _checked_dim, _model_masses, check_symmetric, pair_row_start

        dim = _checked_dim(dim)
        structures, systems = list(structures), list(systems)
        nb = len(structures)
        if nb < 1:
            raise ValueError("a batch needs at least one member")
        if nb > 65535:
            raise ValueError(f"at most 65535 members, got {nb}")
        if not isinstance(force_fields, (list, tuple)):
            force_fields = [force_fields] * nb
        if len(systems) != nb or len(force_fields) != nb:
            raise ValueError(f"{nb} structures, {len(systems)} systems and {len(force_fields)} force fields: the lists must "
                             "have one length")
        if masses is not None and masses is not True and masses is not False and len(masses) != nb:
            raise ValueError(f"{len(masses)} mass entries for {nb} structures")
        coords, parts = [], []
        for b in range(nb):
            try:
                coords.append(_validated_coord(_atoms.coord(structures[b]), force_fields[b]))
                parts.append(_partition(len(coords[b]), systems[b], self._allow_empty_environment))
            except ValueError as e:
                raise ValueError(f"{self._who.format(b)}{e}") from None
        n_s = len(parts[0][0])
        for b in range(nb):
            if len(parts[b][0]) != n_s:
                raise ValueError(f"member {b}: its system has {len(parts[b][0])} atoms, member 0's {n_s}: every member "
                                 "needs one atom per aligned position")
        fit = bool(fit) and dim == 3
        if fit and n_s < 3:
            raise ValueError(f"fit=True needs at least 3 system atoms to superimpose, got {n_s}")
        # per member, for every step below; the public attributes of the same names are these lists
        self._parts = parts
        self._system_index = [p[0] for p in parts]
        self._environment_index = [p[1] for p in parts]
        self._n_env = [len(p[1]) for p in parts]
        self.system_index, self.environment_index, self.n_env = self._system_index, self._environment_index, self._n_env
        self.sizes = [len(c) for c in coords]
        need = max(self._n_env)
        if env_order is None:
            env_order = need
        env_order = int(env_order)
        if env_order < need:
            member = int(np.argmax(self._n_env))
            raise ValueError(f"env_order = {env_order} is below the {need} environment atoms of member {member}")
        if masses is None or masses is False:
            mass = [None] * nb
        elif masses is True:
            mass = [_model_masses(structures[b], True, self.sizes[b]) for b in range(nb)]
        else:
            mass = [_model_masses(structures[b], masses[b], self.sizes[b]) for b in range(nb)]
        self.masses = mass

        self._device_setup(device, nb, n_s, dim, dim * n_s)
        self.env_order, self.m_env = env_order, dim * env_order
        self._hes = self._hee = self._info = None
        self._reduced = False
        torch = self.torch

        self.transforms = self.fit_rmsd = None
        if fit:
            coords = self._fit_members(coords)
        self.fitted_coord = coords

        # the networks: the device scans the contacts, the force fields give the constants on the host, member by member
        pairs_all, gamma_all, starts, self._isolated, self._uncoupled = [], [], [], {}, []
        for b, (coord, ff) in enumerate(zip(coords, force_fields)):
            n, who = self.sizes[b], self._who.format(b)
            pairs, gamma = self._scan_network(coord, ff, who)
            try:
                check_symmetric(pairs, gamma, n)
            except ValueError as e:
                raise ValueError(f"{who}{e}") from None
            group, env = parts[b][2], parts[b][1]
            contacts = np.bincount(pairs[:, 0], minlength=n)
            lonely = env[contacts[env] == 0]
            if len(lonely):
                self._isolated[b] = lonely
            if len(env) and not np.any(group[pairs[:, 0]] != group[pairs[:, 1]]):
                self._uncoupled.append(b)
            pairs_all.append(pairs)
            gamma_all.append(gamma)
            starts.append(pair_row_start(pairs, n))
        self.n_pairs = [len(p) for p in pairs_all]
        atom0 = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        pair0 = np.concatenate([[0], np.cumsum(self.n_pairs)]).astype(np.int64)
        self.offsets = atom0
        # (batch, 5) int64: atom offset, atom count, pair offset, pair count, n_e -- the library stages it at every call
        self._members = np.ascontiguousarray(np.stack([atom0[:-1], self.sizes, pair0[:-1], self.n_pairs, self._n_env], axis=1),
                                             dtype=np.int64)
        ism = None
        if any(mb is not None for mb in mass):
            ism = np.ones((nb, n_s))
            for b, mb in enumerate(mass):
                if mb is not None:
                    ism[b] = 1.0 / np.sqrt(mb[self._system_index[b]])
        with torch.cuda.device(self.device):
            dev = self.device
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            self._coord = up(np.concatenate(coords))
            self._pairs = up(np.concatenate(pairs_all).reshape(-1, 2))
            self._gamma = up(np.concatenate(gamma_all))
            self._row_start = up(np.concatenate(starts))
            self._group = up(np.concatenate([p[2] for p in parts]))
            self._pos = up(np.concatenate([p[3] for p in parts]))
            self.inv_sqrt_mass = None if ism is None else up(ism)
            self.core_coord = up(np.stack([c[s] for c, s in zip(coords, self._system_index)]))

    def _fit_members(self, coords):
        from .ensemble import Ensemble, superimpose

        cores = np.stack([c[s] for c, s in zip(coords, self._system_index)])
        ens = Ensemble(cores, device=self.device.index)
        ens.superpose()
        mean = ens.mean().cpu().numpy()
        _, rmsd, (rot, trans) = superimpose(mean, cores, return_transform=True, device=self.device.index)
        self.transforms, self.fit_rmsd = (rot, trans), rmsd
        return [np.ascontiguousarray(c @ rot[b].T + trans[b]) for b, c in enumerate(coords)]

    def _check_network(self):
        for b, lonely in self._isolated.items():
            shown = ", ".join(str(a) for a in lonely[:10]) + (", ..." if len(lonely) > 10 else "")
            raise ValueError(f"{self._who.format(b)}{len(lonely)} environment atom(s) without any contact ({shown}): H_ee is "
                             "singular")
        if self._uncoupled:
            raise ValueError(f"{self._who.format(self._uncoupled[0])}the system shares no spring with the environment: there "
                             "is nothing to reduce, and the environment's own rigid-body motions make H_ee singular")

    def _check_member(self, member):
        b = int(member)
        if not 0 <= b < self.batch:
            raise ValueError(f"member {member} outside 0..{self.batch - 1}")
        return b

    # ---- assembly, reduction, eigensolve ------------------------------------------------------------------------------------
    def workspace_bytes(self):
        """Context scratch the reduction occupies (0 when every member is exactly the core)."""
        size = C.c_size_t(0)
        self.ctx.check(self._L.sc_dev_vsa_batch_workspace(self.dim, self.n_atoms, self.env_order, self.batch, C.byref(size)))
        return int(size.value)

    def blocks(self):
        """
        ``(H_ss (B, m, m), H_es (B, m_env, m), H_ee (B, m_env, m_env))`` as new CUDA tensors, every entry of every slot
        written: member b's own blocks in the leading ``dim * n_env[b]`` rows / columns, 1.0 on the pad diagonal of H_ee and
        0.0 in every other pad entry.  Only enqueues.
        """
        b = self.batch
        out = self._empty((b, self.m, self.m)), self._empty((b, self.m_env, self.m)), self._empty((b, self.m_env, self.m_env))
        self._blocks_into(*out)
        return out

    def _blocks_into(self, hss, hes, hee):
        p = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())   # noqa: E731
        self.ctx.check(self._L.sc_dev_vsa_batch_blocks_f64(
            self.ctx.handle, _hip.ptr(self._members), self.batch, self.dim, self.n_atoms, self.env_order, p(self._coord),
            p(self._pairs), p(self._gamma), p(self._row_start), p(self._group), p(self._pos), p(self.inv_sqrt_mass), p(hss),
            p(hes), p(hee)))

    def _reduce_into(self, hss):
        """``hss`` (B, m, m) <- H_eff; ``self._hee`` <- the slots' factors, ``self._hes`` <- Y, kept for the follow motion."""
        self._check_network()
        if self._hes is None:
            self._hes = self._empty((self.batch, self.m_env, self.m))
            self._hee = self._empty((self.batch, self.m_env, self.m_env))
            self._info = self.torch.zeros((self.batch,), dtype=self.torch.int64, device=self.device)
        p = lambda t: None if t.numel() == 0 else C.c_void_p(t.data_ptr())   # noqa: E731
        self._blocks_into(hss, self._hes, self._hee)
        self.ctx.check(self._L.sc_dev_vsa_batch_reduce_f64(self.ctx.handle, p(hss), p(self._hes), p(self._hee), self.m, self.m_env,
                                                           self.batch, p(self._info)))
        self._reduced = True
        return hss

    def effective_hessian(self):
        """(B, m, m) CUDA tensor, member b's ``H_ss - H_se H_ee^-1 H_es`` (``T_s ... T_s`` with masses); only enqueues."""
        return self._reduce_into(self._empty((self.batch, self.m, self.m)))

    def _allocate(self, m, nvec, want_vectors=True):
        if self.matrix is None:
            self.matrix = self._empty((self.batch, m, m))
        if self.w is None or self.w.shape[1] != nvec:
            self.w = self._empty((self.batch, nvec))
            self.v = self._empty((self.batch, nvec, m))

    def assemble(self):
        """``self.matrix`` (B, m, m) <- H_eff of every member."""
        self._allocate(self.m, self.nvec)
        self._reduce_into(self.matrix)
        return self.matrix

    def eigh(self):
        """Eigendecomposes ``self.matrix`` (destroyed): (w (B, nvec), v (B, nvec, m))."""
        self._eigh_reduced(self.v)
        return self.w, self.v

    def solve(self, subset_by_index=None):
        """
        Assembly, reduction and eigensolve of all members, enqueued on the device: ``w`` (B, nvec), ``v`` (B, nvec, m).
        ``subset_by_index=(lo, hi)``: only the modes lo..hi (inclusive, ascending) of every member through the
        partial-spectrum solver; row r is then mode ``lo + r``.

        ValueError naming the member before anything is enqueued: an environment atom without any contact, or a member with
        an environment whose system shares no spring with it; either makes H_ee singular.  (A network of several connected
        parts is the caller's to avoid, as for an :class:`ANM`; a factorisation that fails anyway raises LinAlgError in
        :meth:`finish`.)
        """
        self._check_network()
        self._index_subset(subset_by_index)
        self.assemble()
        return self.eigh()

    def eigen(self, subset_by_index=None):
        """Eigenvalues (B, nvec) and modes (B, nvec, m) of every member's H_eff as host arrays."""
        self.solve(subset_by_index)
        w, v = self.finish()
        return w.cpu().numpy(), v.cpu().numpy()

    def finish(self):
        """
        Waits for what was enqueued.  ``np.linalg.LinAlgError`` naming the members whose H_ee was not positive definite
        (their ``H_eff``, ``w`` and ``v`` are NaN; the others are valid); reported once.  Returns (w, v).
        """
        try:
            self.ctx.synchronize()
        except np.linalg.LinAlgError as e:
            info = None if self._info is None else self._info.cpu().numpy()
            failed = [] if info is None else np.nonzero(info)[0]
            if len(failed):
                which = ", ".join(f"{b} (info = {info[b]})" for b in failed)
                raise np.linalg.LinAlgError(f"H_ee of member(s) {which} is not positive definite: their environment can "
                                            f"move freely; the other members' results are valid ({e})") from None
            raise
        return self.w, self.v

    # ---- the environments' motion --------------------------------------------------------------------------------------------
    def environment_displacement(self, member, rows=None):
        """
        ``x_e = -H_ee^-1 H_es x_s`` of one member for its solved modes (``rows=None``: (nvec, dim * n_env[member])) or for
        the q rows of a contiguous CUDA float64 tensor (q, m) of system displacements (in mass-weighted coordinates with
        ``masses``).  A member without environment gives an empty (q, 0) tensor.  Only enqueues.
        """
        return self._follow(self._check_member(member), rows)

    def _follow(self, b, rows):
        if not self._reduced:
            raise ValueError("the follow motion needs the reduction: call solve() or effective_hessian() first")
        if rows is None:
            self._need_vectors()
            rows = self.v[b]
        else:
            q = rows.shape[0] if getattr(rows, "ndim", 0) == 2 else -1
            self._device_f64(rows, (q, self.m), "rows")
            if q < 1:
                raise ValueError(f"Expected rows of shape (q, {self.m}) with q >= 1, got {tuple(rows.shape)}")
        q = rows.shape[0]
        own = self.dim * self._n_env[b]
        if own == 0:
            return self._empty((q, 0))
        out = self._empty((q, self.m_env))
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self.ctx.check(self._L.sc_dev_subsystem_follow_f64(self.ctx.handle, p(self._hee[b]), p(self._hes[b]), self.m, self.m_env,
                                                           p(rows), q, p(out)))
        return out[:, :own].contiguous()

    def full_modes(self, member):
        """
        (nvec, dim * n_b) CUDA tensor of one member: its solved modes at the core atoms and the follow motion at its
        environment atoms, in the member's atom order.  NOT normalised (see :class:`Subsystem`).
        """
        return self._full_modes(self._check_member(member))

    def _full_modes(self, b):
        self._need_vectors()
        torch, d, n = self.torch, self.dim, self.sizes[b]
        xe = self._follow(b, None)
        out = self._empty((self.nvec, n, d))
        out[:, torch.from_numpy(self._system_index[b]).to(self.device)] = self.v[b].view(self.nvec, self.n_atoms, d)
        if self._n_env[b]:
            out[:, torch.from_numpy(self._environment_index[b]).to(self.device)] = xe.view(self.nvec, self._n_env[b], d)
        return out.view(self.nvec, d * n)


class Subsystem(SubsystemBatch):
    """
    Normal modes of a subsystem inside its relaxing environment, on the device: the one-member case of
    :class:`SubsystemBatch`, without a fit and with a slot of exactly the environment's order, so every step is that class's.

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

    _who = ""
    _allow_empty_environment = False   # then there is nothing to reduce: use ANM / GNM

    def __init__(self, atoms, force_field, system, masses=None, dim=3, device=None):
        if masses is not None and masses is not True and masses is not False:
            masses = [masses]
        super().__init__([atoms], [force_field], [system], masses=masses, dim=dim, fit=False, device=device)
        # the public face: one structure's arrays and counts, not lists per member
        self.system_index, self.environment_index, self.group, self.position = self._parts[0]
        self.coord, self.masses = self.fitted_coord[0], self.masses[0]
        self.n_total, self.n_env, self.n_pairs = self.sizes[0], self._n_env[0], self.n_pairs[0]

    def blocks(self):
        """``(H_ss (m, m), H_es (m_env, m), H_ee (m_env, m_env))`` as new CUDA tensors, every entry written; only enqueues."""
        return tuple(t[0] for t in super().blocks())

    def effective_hessian(self):
        """(m, m) CUDA tensor ``H_ss - H_se H_ee^-1 H_es`` (``T_s ... T_s`` with masses), every entry written; only enqueues."""
        return super().effective_hessian()[0]

    def eigen(self, subset_by_index=None):
        """
        Eigenvalues (ascending, shape (nvec,)) and modes (rows, shape (nvec, m)) of H_eff as host arrays, like
        ``ANM.eigen()``: the first dim (dim + 1) / 2 belong to rigid-body motions of the system with its environment.
        """
        w, v = super().eigen(subset_by_index)
        return w[0], v[0]

    #: waits for what was enqueued and raises the context's own ``np.linalg.LinAlgError`` when H_ee was not positive
    #: definite (there is no other member to name); reported once
    finish = _BatchSolver.finish

    def environment_displacement(self, rows=None):
        """
        ``x_e = -H_ee^-1 H_es x_s`` for the solved modes (``rows=None``: (nvec, m_env)) or for the q rows of a contiguous
        CUDA float64 tensor (q, m) of system displacements (in mass-weighted coordinates with ``masses``).  Only enqueues.
        """
        return self._follow(0, rows)

    def full_modes(self):
        """
        (nvec, dim N) CUDA tensor: the solved modes at the system atoms and the follow motion at the environment atoms, in
        the original atom order.  NOT normalised (see the class docstring).
        """
        return self._full_modes(0)

