"""
Rotation-translation blocks (RTB; Durand, Trinquier & Sanejouand 1994, Tama et al. 2000; ProDy's ``RTB``, Bio3D's ``rtb``):
the lowest normal modes of a network too large for its dense Hessian.  Atoms are grouped into rigid blocks, the Hessian is
projected onto the <= 6 rigid-body motions of every block, ``H_b = P^T H P``, the small matrix is solved and its modes are
expanded back, ``v = P u``.  The reference has no counterpart.

:func:`rtb_projector` builds ``P`` on the host (NumPy only); :class:`RTB` projects on the device straight from the pair
list (``csrc/rtb.hip``: the (3N, 3N) Hessian is never formed), solves with the device eigensolver and hands the expanded
modes to the mode consumers it shares with the batch solvers.
"""

import ctypes as C

import numpy as np

from . import atoms as _atoms
from .batch import _ReducedSolver

__all__ = ["RTB", "rtb_projector", "blocks_of_consecutive"]


def blocks_of_consecutive(n_atoms, size):
    """Block labels ``arange(n_atoms) // size``: runs of ``size`` consecutive atoms (the last one may be shorter)."""
    n_atoms, size = int(n_atoms), int(size)
    if n_atoms < 0:
        raise ValueError(f"n_atoms must not be negative, got {n_atoms}")
    if size < 1:
        raise ValueError(f"the block size must be at least 1, got {size}")
    return np.arange(n_atoms) // size


def rtb_projector(coord, blocks, masses=None):
    """
    The block projector of the rotation-translation-block method.

    Parameters
    ----------
    coord : ndarray, shape=(n,3), dtype=float
    blocks : ndarray, shape=(n,)
        Block labels, any integers or strings; atoms with equal labels form a block, contiguous in atom order or not.
        Blocks are numbered in the order of their first appearance.
    masses : ndarray, shape=(n,), dtype=float, optional
        Atomic masses (1 when None).  ``P`` is then orthonormal in mass-weighted coordinates, the space of
        ``ANM(masses=...).hessian``.

    Returns
    -------
    P : ndarray, shape=(n,3,6), dtype=float
        Atom a's three rows of its block's columns: ``P[a, :, c]`` is the atom's part of the block's c-th rigid-body field.
        Per block with atoms A, masses m_a, total mass M and centre of mass c the raw fields are three translations
        ``sqrt(m_a / M) e_x`` and three rotations ``sqrt(m_a) e_x x (r_a - c)``; the rotations, orthogonal to the
        translations about the centre of mass, are orthonormalised by the SVD of their (3 |A|, 3) matrix.  Unused
        columns are exactly 0.0.
    block_of_atom : ndarray, shape=(n,), dtype=int32
    dof : ndarray, shape=(nb,), dtype=int64
        Columns per block: 3 for a one-atom block (decided by the atom count, not by a threshold), else 3 plus the number
        of rotational singular values above ``1e-8 * sqrt(M) * max_a |r_a - c|``: 5 for collinear atoms, 6 otherwise.
    offset : ndarray, shape=(nb+1,), dtype=int64
        Exclusive scan of ``dof``: block b owns the rows ``offset[b] .. offset[b + 1] - 1`` of the projected matrix,
        whose order is ``offset[-1]``.
    """
    coord = np.asarray(coord, dtype=np.float64)
    if coord.ndim != 2 or coord.shape[1] != 3:
        raise ValueError(f"Expected coordinates with shape (n,3), got {coord.shape}")
    n = len(coord)
    if not np.all(np.isfinite(coord)):
        raise ValueError("coordinates must be finite")
    labels = np.asarray(blocks)
    if labels.ndim != 1 or len(labels) != n:
        raise IndexError(f"{labels.shape} block labels for {n} atoms given")
    if masses is None:
        m = np.ones(n)
    else:
        m = np.asarray(masses, dtype=np.float64)
        if m.shape != (n,):
            raise IndexError(f"{m.shape} masses for {n} atoms given")
        if not np.all(m > 0) or not np.all(np.isfinite(m)):
            raise ValueError("Masses must be positive and finite")

    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    block_of_atom = rank[inverse.reshape(-1)]
    nb = len(first)

    P = np.zeros((n, 3, 6))
    dof = np.full(nb, 3, dtype=np.int64)
    members = np.argsort(block_of_atom, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(block_of_atom, minlength=nb))])
    for b in range(nb):
        idx = members[bounds[b]: bounds[b + 1]]
        mb = m[idx]
        total = mb.sum()
        P[idx[:, None], [0, 1, 2], [0, 1, 2]] = np.sqrt(mb / total)[:, None]
        if len(idx) == 1:
            continue
        x = coord[idx] - (mb[:, None] * coord[idx]).sum(axis=0) / total
        # rot[a, :, k] = sqrt(m_a) e_k x x_a
        rot = np.zeros((len(idx), 3, 3))
        rot[:, 1, 0], rot[:, 2, 0] = -x[:, 2], x[:, 1]
        rot[:, 0, 1], rot[:, 2, 1] = x[:, 2], -x[:, 0]
        rot[:, 0, 2], rot[:, 1, 2] = -x[:, 1], x[:, 0]
        rot *= np.sqrt(mb)[:, None, None]
        u, s, _ = np.linalg.svd(rot.reshape(-1, 3), full_matrices=False)
        r = int(np.count_nonzero(s > 1e-8 * np.sqrt(total) * np.sqrt((x * x).sum(axis=1)).max()))
        P[idx, :, 3: 3 + r] = u[:, :r].reshape(len(idx), 3, r)
        dof[b] = 3 + r
    offset = np.concatenate([[0], np.cumsum(dof)]).astype(np.int64)
    return P, block_of_atom.astype(np.int32), dof, offset


class RTB(_ReducedSolver):
    """
    Rotation-translation-block normal modes of one structure on the device.

    Parameters
    ----------
    atoms : AtomArray, shape=(n,) or ndarray, shape=(n,3), dtype=float
    force_field : ForceField, natoms=n
        Any force field, patched and tabulated ones included: the device scans the contacts, ``force_constant()`` gives
        the constants of the ordered pairs on the host, as ``compute_hessian`` does for a user-defined force field.
    blocks : ndarray, shape=(n,)
        Block labels (:func:`rtb_projector`, :func:`blocks_of_consecutive`), e.g. ``chain_id`` joined with ``res_id // 5``.
    masses : bool or ndarray, shape=(n,), dtype=float, optional
        As for :class:`ANM`: the Hessian is mass-weighted and so are the modes.
    device : int, optional

    ``projected_hessian()`` is the (nr, nr) matrix ``P^T H P`` as a CUDA tensor, summed from the pair list in a fixed
    order (two calls agree bit for bit); no (3N, 3N) buffer exists anywhere.  ``solve(subset_by_index=None)`` enqueues
    projection, eigensolve and expansion on torch's current stream and leaves ``w`` (1, nvec) and ``v`` (1, nvec, 3N), rows =
    modes in the Hessian's own (mass-weighted) coordinates, the six rigid-body modes first as for an :class:`ANM`;
    ``eigen()`` returns them as host arrays.  The modes are the Ritz pairs of the Hessian in the block space: ``w[k]`` is
    never below the k-th eigenvalue of the full Hessian.

    After a solve every mode consumer of the batch solvers works on the RTB modes, with a leading batch axis of one:
    ``frequencies``, ``mean_square_fluctuation``, ``bfactor``, ``dcc``, ``anisotropic_fluctuation``, ``overlap``,
    ``collectivity``, ``distance_fluctuation``, ``linear_response``, ``mode_displacement``.  ``mode_subset`` holds global
    mode indices of the block spectrum, 6 .. nr - 1.

    How good the block modes are can be read without the dense problem: ``operator`` is the Hessian as a
    :class:`~springcraft_amd.PairOperator` on the solver's own pair list (no second contact scan), ``residuals()`` gives
    ``|H v_k - w_k v_k|`` per solved row -- some exact eigenvalue of the full Hessian lies within it of ``w[k]`` --
    and ``deformation_energy()`` / ``spring_strain()`` say where a mode strains the network.  They need symmetric force
    constants (ValueError otherwise).

    ``projector`` (n, 3, 6), ``block_of_atom`` (n,), ``dof`` (nb,) and ``offset`` (nb + 1,) are the host arrays of
    :func:`rtb_projector`; ``nr = offset[-1]``.
    """

    def __init__(self, atoms, force_field, blocks, masses=None, device=None):
        from .interaction import _validated_coord

        coord = _validated_coord(_atoms.coord(atoms), force_field)
        n = len(coord)
        if masses is None or masses is False:
            mass = None
        elif masses is True:
            from ._model import residue_mass

            if not _atoms.is_atom_array(atoms):
                raise TypeError("An AtomArray is required to automatically infer masses")
            mass = np.array([residue_mass(r) for r in atoms.res_name], dtype=np.float64)
        else:
            mass = np.array(masses, dtype=np.float64)
            if mass.shape != (n,):
                raise IndexError(f"{mass.shape} masses for {n} atoms given")
        self.projector, self.block_of_atom, self.dof, self.offset = rtb_projector(coord, blocks, mass)
        self.masses = mass
        self.coord = coord
        self.n_atoms, self.n_blocks, self.nr = n, len(self.dof), int(self.offset[-1])

        self._device_setup(device, 1, n, 3, self.nr)
        self._u = None
        self._operator = None
        self._refined = False   # whether w and v are exact eigenpairs: after a refine() that converged

        pairs, gamma = self._scan_network(coord, force_field)
        self.n_pairs = len(pairs)
        self._isolated = np.nonzero(np.bincount(pairs[:, 0], minlength=n) == 0)[0]

        torch = self.torch
        with torch.cuda.device(self.device):
            dev, i64 = self.device, torch.int64
            self._coord = torch.from_numpy(coord).to(dev)
            self._P = torch.from_numpy(self.projector).to(dev)
            self._boa = torch.from_numpy(self.block_of_atom).to(dev)
            self._offset = torch.from_numpy(self.offset).to(dev)
            self._pairs = torch.from_numpy(pairs).to(dev)
            self._gamma = torch.from_numpy(gamma).to(dev)
            self.inv_sqrt_mass = None if mass is None else torch.from_numpy(1.0 / np.sqrt(mass)).to(dev)[None, :].contiguous()
            # the order of the sums: pairs sorted by (block of the second atom, block of the first), stable, with the
            # starts of the runs of equal keys and of every block of the second atom
            nb = self.n_blocks
            boa = self._boa.to(i64)
            key = boa[self._pairs[:, 1]] * nb + boa[self._pairs[:, 0]]
            key, self._order = torch.sort(key, stable=True)
            first = torch.ones(len(key), dtype=torch.bool, device=dev)
            first[1:] = key[1:] != key[:-1]
            seg = torch.nonzero(first).flatten()
            self._seg_start = torch.cat([seg, torch.tensor([len(key)], dtype=i64, device=dev)])
            self.n_segments = len(seg)
            self._block_start = torch.searchsorted(key, torch.arange(nb + 1, dtype=i64, device=dev) * nb)

    # ---- projection, eigensolve, expansion -------------------------------------------------------------------------
    def _project(self, out):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        self.ctx.check(self._L.sc_dev_rtb_hessian_f64(
            self.ctx.handle, p(self._coord), self.n_atoms, p(self._pairs), self.n_pairs, p(self._gamma),
            p(self.inv_sqrt_mass), p(self._P), p(self._boa), p(self._offset), self.n_blocks, self.nr, p(self._order),
            p(self._seg_start), self.n_segments, p(self._block_start), p(out)))
        return out

    def projected_hessian(self):
        """(nr, nr) CUDA tensor ``P^T H P``, every entry written; only enqueues."""
        return self._project(self._empty((self.nr, self.nr)))

    def _allocate(self, m, nvec, want_vectors=True):
        """The tensors of a solve; ``m`` is the block order nr: no (3N, 3N) tensor exists."""
        if self.matrix is None:
            self.matrix = self._empty((1, m, m))
        if self.w is None or self.w.shape[1] != nvec:
            self.w = self._empty((1, nvec))
            self._u = self._empty((1, nvec, m))
            self.v = self._empty((1, nvec, 3 * self.n_atoms))

    def assemble(self):
        """``self.matrix`` (1, nr, nr) <- the projected Hessian."""
        self._allocate(self.nr, self.nvec)
        self._project(self.matrix)
        return self.matrix

    def eigh(self):
        """Eigendecomposes ``self.matrix`` (destroyed) and expands the block modes: (w (1, nvec), v (1, nvec, 3N))."""
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self._eigh_reduced(self._u)
        self.ctx.check(self._L.sc_dev_rtb_expand_f64(self.ctx.handle, p(self._u), self.nvec, self.nr, p(self._P),
                                                     p(self._boa), p(self._offset), self.n_atoms, p(self.v)))
        return self.w, self.v

    def solve(self, subset_by_index=None):
        """
        Projection, eigensolve and expansion, all enqueued on the device: ``w`` (1, nvec), ``v`` (1, nvec, 3N).  Call
        :meth:`finish` before trusting them on the host.  ``subset_by_index=(lo, hi)``: only the block modes lo..hi
        (inclusive, ascending) through the partial-spectrum solver; row r is then mode ``lo + r``.

        An atom without a contact makes more than six modes trivial, and the consumers would divide by rounding-level
        eigenvalues: that raises ValueError naming the atoms, before anything is enqueued.  (Only atoms without any
        contact are looked for; a network of several connected parts is the caller's to avoid, as for an :class:`ANM`.)
        """
        if len(self._isolated):
            shown = ", ".join(str(a) for a in self._isolated[:10]) + (", ..." if len(self._isolated) > 10 else "")
            raise ValueError(f"{len(self._isolated)} atom(s) without any contact ({shown}): the block network has more "
                             "than six trivial modes")
        self._index_subset(subset_by_index)
        self.assemble()
        self._refined = False   # (block modes again)
        return self.eigh()

    def eigen(self, subset_by_index=None):
        """
        Eigenvalues (ascending, shape (nvec,)) and modes (rows, shape (nvec, 3n)) of the block-projected Hessian as host
        arrays, like ``ANM.eigen()``: the first six belong to rigid-body motions.
        """
        self.solve(subset_by_index)
        w, v = self.finish()
        return w[0].cpu().numpy(), v[0].cpu().numpy()

    # ---- the Hessian as an operator on the solver's pair list (pair_operator.py) ------------------------------------------
    @property
    def operator(self):
        """The (mass-weighted) Hessian as a :class:`~springcraft_amd.PairOperator` on this solver's pairs, constants and context."""
        if self._operator is None:
            from .pair_operator import PairOperator

            ism = None if self.inv_sqrt_mass is None else self.inv_sqrt_mass[0]
            self._operator = PairOperator.from_pairs(self._coord, self._pairs, self._gamma, dim=3, inv_sqrt_mass=ism,
                                                     _ctx=self.ctx)
        return self._operator

    def _mode_rows(self, mode_subset, trivial=False):
        """(w, v) of the rows a mode_subset names; None: every solved row, the trivial ones only with ``trivial``."""
        self._need_vectors()
        if mode_subset is None and trivial:
            return self.w[0], self.v[0]
        from .batch import batch_mode_rows

        rows = batch_mode_rows(mode_subset, self._ntriv, self.subset, self._common_modes, self.window)
        rows = self.torch.from_numpy(rows.astype(np.int64)).to(self.device)
        return self.w[0][rows], self.v[0][rows]

    def residuals(self, mode_subset=None):
        """
        ``|H v_k - w_k v_k|_2`` of the solved pairs against the full Hessian, a CUDA tensor (nvec,) for ``mode_subset=None``
        (every solved row, the trivial ones included), else one per listed mode (global indices as for the other
        consumers).  The modes are unit vectors, so an exact eigenvalue lies within ``residuals()[k]`` of ``w[k]``; a
        small residual also bounds the mode's angle to the exact eigenspace by residual / gap.  Only enqueues.
        """
        w, v = self._mode_rows(mode_subset, trivial=True)
        return self.operator.residual(w, v)

    def deformation_energy(self, mode_subset=None):
        """
        (k, n_atoms) CUDA tensor of Hinsen's per-atom deformation energies of the selected block modes
        (:func:`nma.deformation_energy`); a row sums to ``<v_k, H v_k> = w[k]``.  None: every solved non-trivial mode.
        """
        return self.operator.energy(self._mode_rows(mode_subset)[1])

    def spring_strain(self, mode_subset=None):
        """
        ``(springs, strain)``: ``springs`` (P, 2) host array of the contacts with ``i < j``, ``strain`` (k, P) CUDA tensor
        ``gamma_s e_s^2`` of the selected block modes (:func:`nma.spring_strain`); a row sums to ``w[k]``.
        """
        op = self.operator
        return op.springs, op.strain(self._mode_rows(mode_subset)[1])

    def refine(self, tol=1e-8, **options):
        """
        Replaces the block modes of the last :meth:`solve` by eigenpairs of the full (mass-weighted) Hessian for the same
        rows: :meth:`PairOperator.lowest_modes` started from ``self.v``, to residuals ``<= tol * b``
        (``options``: ``degree``, ``guard``, ``max_iter``, ``seed``).  ``self.w`` (1, nvec) and ``self.v`` (1, nvec, 3N)
        are replaced, so every mode consumer and :meth:`residuals` then work on the refined modes; ``eigen()`` and
        ``solve()`` give block modes again.  Returns the solver's info record (``converged``, ``iterations``,
        ``panel_steps``, ``residuals``, ``b``).  The iteration finds the LOWEST modes: it is defined for a solve whose rows
        start at mode 0, ``subset_by_index=(0, hi)`` or the full block spectrum, and raises ValueError otherwise.
        """
        self._need_vectors()
        if self._first_row != 0:
            raise ValueError(f"refine() finds the lowest modes and needs a solve whose rows start at mode 0, not at "
                             f"{self._first_row}: solve(subset_by_index=(0, hi))")
        if "start" in options:
            raise ValueError("refine() starts from the block modes")
        w, v, info = self.operator.lowest_modes(self.nvec, start=self.v[0], tol=tol, **options)
        self.w, self.v = w[None, :], v[None, :, :]
        self._refined = bool(info["converged"])
        return info

    def exact_response(self, force, tol=1e-8, deflate=True, **options):
        """
        The Cartesian displacement a force induces from the EXACT pseudo-inverse of the full Hessian,
        :meth:`PairOperator.linear_response` on :attr:`operator` (conjugate gradients on the pair list): ``(x, info)``, ``x`` a
        CUDA tensor (n, 3) or (q, n, 3) for a force (n, 3), (3n,) or (q, n, 3).  :meth:`linear_response` sums over the solved
        modes only and leaves out every mode above them.  With ``deflate`` the solver's own ``w`` and ``v`` serve as the
        deflation space when they are exact eigenpairs, that is after a :meth:`refine` that converged; block modes are
        not, and the solve then runs undeflated.  ``options``: ``max_iter``, ``check_every``.
        """
        if "deflate" in options:
            raise ValueError("exact_response() deflates with the solver's own modes: deflate=True or False")
        space = (self.w[0], self.v[0]) if deflate and self._refined and self.v is not None else None
        return self.operator.linear_response(force, tol=tol, deflate=space, **options)
