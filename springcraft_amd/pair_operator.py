"""
The Hessian / Kirchhoff matrix of an elastic network as an operator on its ordered pair list (``csrc/pair_operator.hip``):
products ``H x``, Rayleigh quotients, residuals of approximate eigenpairs, per-atom deformation energies (Hinsen 1998;
Bio3D's ``deformation.nma``) and per-spring strain, without the (dim N, dim N) matrix.  The reference has no counterpart.

For a row ``x`` of length dim N, the atom scale ``t_a`` (``1 / sqrt(mass)``, or 1), ``u[a] = t_a x[dim a .. dim a + dim - 1]``
and the directed pair p = (i, j) with constant ``gamma_p`` and direction ``n_p = (x_j - x_i) / |x_j - x_i|``::

    dim 3:  e_p = n_p . (u[i] - u[j])            dim 1:  e_p = u[i] - u[j]
    Y[i]  = t_i sum_{p = (i, .)} gamma_p e_p n_p  (dim 1: without n_p)      Y = (T H T) x, the matrix the solvers decompose
    E[i]  = 1/2 sum_{p = (i, .)} gamma_p e_p^2                              sum_i E[i] = x^T (T H T) x
    S[p]  = gamma_p e_p^2                                                   sum_p S[p] = 2 x^T (T H T) x

``panel_step`` is one fused step ``Z <- alpha (T H T) X + beta X + gamma_c Z`` on column panels (``csrc/pair_panel.hip``),
``lowest_modes`` the Chebyshev-filtered subspace iteration built on it (:mod:`springcraft_amd.iterative`): the exact lowest
eigenpairs of the matrix to a requested tolerance, in memory of order (dim N, k).  ``solve`` is the inverse direction,
``(T H T)^+ f`` by conjugate gradients on the range of the matrix (``csrc/pair_cg.hip``, :func:`iterative.conjugate_gradient`);
``linear_response`` and ``covariance_columns`` are its consumers.

The constants must be symmetric, ``gamma(i, j) = gamma(j, i)``: the reference's rule for asymmetric ones (off-diagonal
from ``gamma(i, j)``, diagonal summed over the first index) has no energy reading, and :class:`PairOperator` raises
ValueError for them.

:func:`pair_row_start`, :func:`check_symmetric` and :func:`undirected` are host NumPy and need no GPU.
"""

import ctypes as C

import numpy as np

from . import _hip, atoms as _atoms

__all__ = ["PairOperator", "pair_row_start", "check_symmetric", "undirected"]


def _checked_pairs(pairs, n_atoms):
    n_atoms = int(n_atoms)
    if n_atoms < 1:
        raise ValueError(f"n_atoms must be positive, got {n_atoms}")
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"Expected pairs with shape (k,2), got {p.shape}")
    if len(p) and p.dtype.kind not in "iu":
        raise ValueError("pairs must hold integer atom indices")
    p = np.ascontiguousarray(p, dtype=np.int64)
    if len(p) and (p.min() < 0 or p.max() >= n_atoms):
        raise ValueError(f"pairs hold an atom index outside 0..{n_atoms - 1}")
    return p, n_atoms


def pair_row_start(pairs, n_atoms):
    """
    Where every atom's rows start in an ordered pair list: (n_atoms + 1,) int64, atom i owns the rows
    ``row_start[i] .. row_start[i + 1] - 1`` (an atom without pairs has an empty range), ``row_start[-1] = k``.
    ``pairs`` (k, 2) must be sorted by its first column, as ``compute_hessian`` returns it; otherwise ValueError.
    """
    p, n_atoms = _checked_pairs(pairs, n_atoms)
    if len(p) > 1 and np.any(p[1:, 0] < p[:-1, 0]):
        raise ValueError("pairs must be sorted by their first atom")
    start = np.zeros(n_atoms + 1, dtype=np.int64)
    np.cumsum(np.bincount(p[:, 0], minlength=n_atoms), out=start[1:])
    return start


def check_symmetric(pairs, gamma, n_atoms):
    """
    Raises ValueError unless the ordered pair list (sorted by first then second atom, no row twice, no atom with itself)
    holds both directions of every pair with equal constants, ``gamma(i, j) == gamma(j, i)`` exactly.
    """
    p, n_atoms = _checked_pairs(pairs, n_atoms)
    g = np.asarray(gamma, dtype=np.float64)
    if g.shape != (len(p),):
        raise ValueError(f"Expected {len(p)} force constants, one per pair, got shape {g.shape}")
    if not len(p):
        return
    if np.any(p[:, 0] == p[:, 1]):
        raise ValueError("a pair of an atom with itself")
    key = p[:, 0] * n_atoms + p[:, 1]
    if np.any(key[1:] <= key[:-1]):
        raise ValueError("pairs must be sorted by first then second atom, without repeated rows")
    back = p[:, 1] * n_atoms + p[:, 0]
    pos = np.minimum(np.searchsorted(key, back), len(p) - 1)
    missing = np.nonzero(key[pos] != back)[0]
    if len(missing):
        i, j = p[missing[0]]
        raise ValueError(f"pair ({i}, {j}) is listed without its reverse ({j}, {i})")
    differ = np.nonzero(~((g[pos] == g) | (np.isnan(g[pos]) & np.isnan(g))))[0]
    if len(differ):
        i, j = p[differ[0]]
        raise ValueError(f"asymmetric force constants: gamma({i}, {j}) = {float(g[differ[0]])!r} but gamma({j}, {i}) = "
                         f"{float(g[pos[differ[0]]])!r}; products, energies and strain need gamma(i, j) = gamma(j, i)")


def undirected(pairs):
    """Indices (int64) of the rows with ``i < j`` of a directed pair list (k, 2): every spring once, in list order."""
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"Expected pairs with shape (k,2), got {p.shape}")
    return np.nonzero(p[:, 0] < p[:, 1])[0].astype(np.int64)


def _checked_dim(dim):
    if dim not in (1, 3):
        raise ValueError(f"dim must be 1 (GNM) or 3 (ANM), got {dim!r}")
    return int(dim)


def _model_masses(atoms, masses, n):
    """``masses`` as :class:`ANM` takes it -> (n,) float64 array or None."""
    if masses is None or masses is False:
        return None
    if masses is True:
        from ._model import residue_mass

        if not _atoms.is_atom_array(atoms):
            raise TypeError("An AtomArray is required to automatically infer masses")
        return np.array([residue_mass(r) for r in atoms.res_name], dtype=np.float64)
    mass = np.array(masses, dtype=np.float64)
    if mass.shape != (n,):
        raise IndexError(f"{mass.shape} masses for {n} atoms given")
    if np.any(mass == 0):
        raise ValueError("Masses must not be 0")
    return mass


class PairOperator:
    """
    The network's matrix as an operator on the device.

    Parameters
    ----------
    atoms : AtomArray, shape=(n,) or ndarray, shape=(n,3), dtype=float
    force_field : ForceField, natoms=n
        Any force field: the device scans the contacts, ``force_constant()`` gives the constants of the ordered pairs on
        the host, as for :class:`RTB`.  Asymmetric constants raise ValueError.
    dim : 1 or 3
        1: the Kirchhoff matrix of a :class:`GNM`; 3: the Hessian of an :class:`ANM`.
    masses : bool or ndarray, shape=(n,), dtype=float, optional
        As for :class:`ANM`: the operator is then the mass-weighted matrix ``T H T``, ``T = diag(1 / sqrt(mass))``.
    device : int, optional

    Every method takes a (dim n,) or (q, dim n) NumPy array or CUDA float64 tensor -- rows in the coordinates of the
    matrix, as ``eigen()`` returns modes -- enqueues on the stream that was torch's current one at construction and
    returns CUDA tensors with the same leading shape.  An atom's sums run in an order its own pairs fix: a row's result
    does not depend, bit for bit, on the other rows or on how many there are.

    ``n_atoms``, ``n_pairs`` (directed rows), ``dim``; ``pairs`` (k, 2) and ``gamma`` (k,) are the host arrays of the
    directed list, ``springs`` (P, 2) its rows with ``i < j`` (``spring_index`` their positions).
    """

    def __init__(self, atoms, force_field, dim=3, masses=None, device=None):
        from .forcefield import device_plan
        from .interaction import _normalised_patch, _pair_list, _validated_coord

        dim = _checked_dim(dim)
        coord = _validated_coord(_atoms.coord(atoms), force_field)
        n = len(coord)
        mass = _model_masses(atoms, masses, n)
        ctx, dev = self._context(device)
        ff_desc, patch, _ = device_plan(force_field)
        keep = []
        patch_desc = _normalised_patch(patch, n, keep)
        pairs, sq_dist = _pair_list(ctx, coord, ff_desc, patch_desc, want_sq_dist=True)
        gamma = np.ascontiguousarray(force_field.force_constant(pairs[:, 0], pairs[:, 1], sq_dist), dtype=np.float64)
        if gamma.shape != (len(pairs),):
            raise ValueError(f"force_constant() returned shape {gamma.shape} for {len(pairs)} pairs")
        self._adopt(ctx, dev, coord, pairs, gamma, dim, None if mass is None else 1.0 / np.sqrt(mass), n)

    @classmethod
    def from_pairs(cls, coord, pairs, gamma, dim=3, inv_sqrt_mass=None, device=None, n_atoms=None, _ctx=None):
        """
        The operator of an existing pair list: ``coord`` (n, 3) (None for ``dim=1``, which then needs ``n_atoms``),
        ``pairs`` (k, 2) integer, sorted by first then second atom with both directions (what ``compute_hessian``
        returns), ``gamma`` (k,), ``inv_sqrt_mass`` (n,) or None -- host arrays or CUDA tensors, which are adopted as
        they are when they are contiguous, of the right dtype and on the operator's device.  The list is checked on the
        host (order, both directions, symmetric constants; ValueError otherwise).
        """
        import torch

        dim = _checked_dim(dim)
        host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)   # noqa: E731
        if coord is None:
            if dim == 3:
                raise ValueError("dim 3 needs the coordinates")
            if n_atoms is None:
                raise ValueError("without coordinates n_atoms must be given")
            n = int(n_atoms)
        else:
            if tuple(coord.shape) != (len(coord), 3):
                raise ValueError(f"Expected coordinates with shape (n,3), got {tuple(coord.shape)}")
            n = len(coord)
            if n_atoms is not None and int(n_atoms) != n:
                raise ValueError(f"n_atoms = {n_atoms} but {n} coordinates")
        if inv_sqrt_mass is not None and tuple(inv_sqrt_mass.shape) != (n,):
            raise IndexError(f"{tuple(inv_sqrt_mass.shape)} mass factors for {n} atoms given")
        self = cls.__new__(cls)
        ctx, dev = (_ctx, torch.device("cuda", _ctx.device)) if _ctx is not None else self._context(device)
        self._adopt(ctx, dev, coord, pairs, gamma, dim, inv_sqrt_mass, n, host=host)
        return self

    @staticmethod
    def _context(device):
        import torch

        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        return _hip.Context(dev.index, stream=torch.cuda.current_stream(dev).cuda_stream), dev

    def _adopt(self, ctx, dev, coord, pairs, gamma, dim, inv_sqrt_mass, n, host=np.asarray):
        import torch

        self.torch, self.device, self.ctx, self._L = torch, dev, ctx, _hip.lib()
        self.dim, self.n_atoms, self.m = dim, int(n), dim * int(n)
        self.pairs, _ = _checked_pairs(host(pairs), n)
        self.gamma = np.ascontiguousarray(host(gamma), dtype=np.float64)
        check_symmetric(self.pairs, self.gamma, n)
        self.n_pairs = len(self.pairs)
        self.spring_index = undirected(self.pairs)
        self.springs = self.pairs[self.spring_index]

        def dev_of(t, dtype, fallback):
            """The caller's tensor when it can be used as it is, else a device copy of the checked host array."""
            if (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype
                    and t.is_contiguous()):
                return t
            return None if fallback is None else torch.from_numpy(np.ascontiguousarray(fallback)).to(dev)

        with torch.cuda.device(dev):
            self._coord = None if coord is None else dev_of(coord, torch.float64,
                                                            np.asarray(host(coord), dtype=np.float64))
            self._pairs = dev_of(pairs, torch.int64, self.pairs)
            self._gamma = dev_of(gamma, torch.float64, self.gamma)
            self._scale = None
            if inv_sqrt_mass is not None:
                self._scale = dev_of(inv_sqrt_mass, torch.float64, np.asarray(host(inv_sqrt_mass), dtype=np.float64))
            self._row_start = torch.from_numpy(pair_row_start(self.pairs, n)).to(dev)
            self._spring_index = torch.from_numpy(self.spring_index).to(dev)
            self._all_index = None

    # ---- the C entries ------------------------------------------------------------------------------------------------
    def _rows(self, x):
        """``x`` as a contiguous CUDA float64 tensor (q, dim n) on the operator's device, and whether it was one vector."""
        torch = self.torch
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        if x.ndim not in (1, 2) or x.shape[-1] != self.m:
            raise ValueError(f"Expected rows of shape ({self.m},) or (q, {self.m}), got {tuple(x.shape)}")
        single = x.ndim == 1
        x = x.to(device=self.device, dtype=torch.float64)
        return (x[None] if single else x).contiguous(), single

    def _empty(self, shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.device)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _apply(self, x, want_y, want_e):
        x, single = self._rows(x)
        q, p = len(x), self._p
        with self.torch.cuda.device(self.device):
            y = self._empty((q, self.m)) if want_y else None
            e = self._empty((q, self.n_atoms)) if want_e else None
            have = self.n_pairs > 0
            self.ctx.check(self._L.sc_dev_pairs_apply_f64(
                self.ctx.handle, p(self._coord), self.n_atoms, self.dim, p(self._pairs) if have else None, self.n_pairs,
                p(self._gamma) if have else None, p(self._row_start), p(self._scale), p(x) if q else None, q, p(y), p(e)))
        self._keep = x   # (the rows outlive the enqueued call)
        pick = lambda t: None if t is None else (t[0] if single else t)   # noqa: E731
        return pick(y), pick(e)

    def apply(self, x):
        """``(T H T) x`` per row: a CUDA tensor shaped like ``x``."""
        return self._apply(x, True, False)[0]

    def energy(self, x):
        """Per-atom deformation energies ``E[a] = 1/2 sum_c gamma_ac e_ac^2`` per row, (q, n) or (n,): they sum to ``x^T (T H T) x``."""
        return self._apply(x, False, True)[1]

    def apply_energy(self, x):
        """(:meth:`apply`, :meth:`energy`) of the same rows from one pass over the pair list."""
        return self._apply(x, True, True)

    def strain(self, x, pair_index=None):
        """
        ``S[p] = gamma_p e_p^2`` per row for the listed rows of the directed pair list, (q, len(pair_index)) or
        (len(pair_index),): the energy of the spring, and for an eigenvector ``d lambda / d ln gamma_p`` with both
        directions of the spring changed together.  ``pair_index=None`` takes every spring once, the rows with ``i < j``:
        column s belongs to ``springs[s]``.  An index outside ``0 .. n_pairs - 1`` gives a NaN column.
        """
        torch = self.torch
        x, single = self._rows(x)
        with torch.cuda.device(self.device):
            if pair_index is None:
                idx = self._spring_index
            elif isinstance(pair_index, torch.Tensor):
                idx = pair_index.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            else:
                host = np.asarray(pair_index)
                if host.size and host.dtype.kind not in "iu":
                    raise IndexError("pair_index must hold integer row numbers of the pair list")
                idx = torch.from_numpy(np.ascontiguousarray(host.reshape(-1), dtype=np.int64)).to(self.device)
            q, ks, p = len(x), len(idx), self._p
            out = self._empty((q, ks))
            have = self.n_pairs > 0
            self.ctx.check(self._L.sc_dev_pairs_strain_f64(
                self.ctx.handle, p(self._coord), self.n_atoms, self.dim, p(self._pairs) if have else None, self.n_pairs,
                p(self._gamma) if have else None, p(self._scale), p(idx) if ks else None, ks, p(x) if q else None, q,
                p(out) if q and ks else None))
        self._keep = (x, idx)
        return out[0] if single else out

    def rayleigh(self, x):
        """Rayleigh quotients ``<x, H x> / <x, x>`` per row, (q,) or a 0-d tensor."""
        xr, single = self._rows(x)
        r = (xr * self.apply(xr)).sum(dim=1) / (xr * xr).sum(dim=1)
        return r[0] if single else r

    def residual(self, w, x):
        """
        ``|H x_r - w_r x_r|_2`` per row for the approximate eigenpairs ``(w_r, x_r)``, (q,) or a 0-d tensor; ``w`` is a
        number, a (q,) array or a tensor.  For a unit ``x_r`` some exact eigenvalue lies within the residual of ``w_r``.
        """
        torch = self.torch
        xr, single = self._rows(x)
        if not isinstance(w, torch.Tensor):
            w = torch.from_numpy(np.atleast_1d(np.asarray(w, dtype=np.float64)))
        w = w.to(device=self.device, dtype=torch.float64).reshape(-1)
        if len(w) not in (1, len(xr)):
            raise ValueError(f"Expected {len(xr)} eigenvalues, one per row, got {len(w)}")
        r = torch.linalg.vector_norm(self.apply(xr) - w[:, None] * xr, dim=1)
        return r[0] if single else r

    # ---- column panels and the iterative solver (iterative.py, csrc/pair_panel.hip) -------------------------------------
    def spectral_bound(self):
        """``b = 2 max_i t_i^2 sum_{p = (i, .)} |gamma_p|``, an upper bound of the largest eigenvalue (:func:`iterative.spectral_bound`)."""
        from .iterative import spectral_bound

        scale = None if self._scale is None else self._scale.cpu().numpy()
        return spectral_bound(self.pairs, self.gamma, self.n_atoms, scale)

    def panel_step(self, X, Z, alpha, beta, gamma_c):
        """
        ``Z <- alpha (T H T) X + beta X + gamma_c Z`` in place, one kernel; returns ``Z``.  ``X`` and ``Z`` are CUDA float64
        tensors of shape (dim n, q) with strides (ld, 1), ld >= q, the same ld for both: columns are the vectors, the
        transpose of what :meth:`apply` takes.  ``Z`` must not share memory with ``X`` and is read only when
        ``gamma_c != 0``.  A column's bits depend neither on q nor on ld nor on the other columns; the sums run in another
        order than :meth:`apply`'s, whose result they match to rounding.  Only enqueues.
        """
        torch = self.torch
        for name, t in (("X", X), ("Z", Z)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == torch.float64):
                raise ValueError(f"{name} must be a CUDA float64 tensor on {self.device}")
            if t.ndim != 2 or t.shape[0] != self.m:
                raise ValueError(f"Expected a panel of shape ({self.m}, q), got {tuple(t.shape)}")
        q = X.shape[1]
        if Z.shape[1] != q:
            raise ValueError(f"X has {q} columns, Z {Z.shape[1]}")
        ld = X.stride(0) if self.m > 1 else max(q, 1)
        if q == 0:
            return Z
        if (q > 1 and (X.stride(1) != 1 or Z.stride(1) != 1)) or (self.m > 1 and (Z.stride(0) != ld or ld < q)):
            raise ValueError(f"panels need strides (ld, 1) with one ld >= q, got {X.stride()} and {Z.stride()}")
        p, have = self._p, self.n_pairs > 0
        with torch.cuda.device(self.device):
            self.ctx.check(self._L.sc_dev_pairs_panel_f64(
                self.ctx.handle, p(self._coord), self.n_atoms, self.dim, p(self._pairs) if have else None, self.n_pairs,
                p(self._gamma) if have else None, p(self._row_start), p(self._scale), p(X), p(Z), ld, q, float(alpha),
                float(beta), float(gamma_c)))
        return Z

    def _small_eigh(self, a):
        """(w, U) of a symmetric (n, n) CUDA tensor through the device eigensolver; eigenvectors as columns; ``a`` is destroyed."""
        n, p = len(a), self._p
        a = a.contiguous()
        w, v = self._empty((n,)), self._empty((n, n))
        self.ctx.check(self._L.sc_dev_eigh_f64(self.ctx.handle, p(a), n, 1, p(w), p(v)))
        return w, v.T

    def lowest_modes(self, k, start=None, tol=1e-8, degree=20, guard=None, max_iter=100, seed=0):
        """
        The k lowest eigenpairs of ``T H T`` by Chebyshev-filtered subspace iteration
        (:func:`iterative.chebyshev_subspace_iteration`), to residuals ``|H v - w v| <= tol * b`` with ``b`` the
        :meth:`spectral_bound`: ``(w (k,), v (k, dim n), info)``, CUDA tensors, ``w`` ascending, the modes as orthonormal
        rows with the trivial ones first, as everywhere in the package.  No (dim n, dim n) matrix exists; the memory is a
        few panels of ``nb = k + guard`` columns.

        ``start`` (k', dim n), k' >= 1: rows to start from (an array or a tensor), e.g. RTB modes; they are truncated to
        nb, or padded with standard-normal columns of ``RandomState(seed)``; None: all random.  ``guard`` columns beyond
        k keep the wanted end of the block converging (default ``max(8, ceil(k / 4))``, :func:`iterative.default_guard`),
        ``degree`` is that of the filter, ``max_iter`` the most filter passes.  ``info`` holds ``iterations``,
        ``panel_steps``, ``residuals`` (k,), ``b``, ``tol`` and ``converged``; a solve that runs out of passes returns what
        it has with ``converged = False`` and does not raise.  The same arguments give the same bits.
        """
        from . import iterative

        k, guard, nb = iterative.checked_block(k, guard, self.m)
        if int(degree) < 1 or int(max_iter) < 0:
            raise ValueError(f"degree must be at least 1 and max_iter not negative, got {degree} and {max_iter}")
        import torch

        if isinstance(start, torch.Tensor):
            start = start.detach().cpu().numpy()
        x0 = iterative.start_block(start, self.m, nb, seed)   # (every refusal above and here needs no device)
        b = self.spectral_bound()
        with torch.cuda.device(self.device):
            w, x, info = iterative.chebyshev_subspace_iteration(self.panel_step, self._small_eigh,
                                                                torch.from_numpy(x0).to(self.device), k, b, tol=tol,
                                                                degree=int(degree), max_iter=int(max_iter))
            return w.contiguous(), x.T.contiguous(), info

    # ---- the pseudo-inverse by conjugate gradients (iterative.py, csrc/pair_cg.hip) --------------------------------------
    #: The most columns one CG run holds: two chunks of 64 lanes, the width the panel step was measured at.  A solve of q
    #: right-hand sides runs ceil(q / 128) times on five panels (X, R, P, Q and one temporary of the projections) of
    #: ``8 * dim n * 128`` bytes each -- 770 MB at n = 50 000 -- whatever q is.
    SOLVE_COLUMNS = 128

    def null_space(self):
        """The orthonormal null space of a connected network, a CUDA tensor (dim n, z) (:func:`iterative.null_space`); cached."""
        if getattr(self, "_null", None) is None:
            from .iterative import null_space

            coord = self.n_atoms if self._coord is None else self._coord.cpu().numpy()
            scale = None if self._scale is None else self._scale.cpu().numpy()
            self._null = self.torch.from_numpy(null_space(coord, self.dim, scale)).to(self.device)
        return self._null

    def _cg_callables(self, q):
        """(init, step) of :func:`iterative.conjugate_gradient` for panels of q columns on the C entries."""
        torch, L, p = self.torch, self._L, self._p
        size = C.c_size_t()
        if L.sc_dev_pairs_cg_workspace(self.n_atoms, q, C.byref(size)) != _hip.SC_OK:
            raise ValueError(f"no CG workspace for {self.n_atoms} atoms and {q} columns")
        work = torch.empty(max(size.value // 8, 1), dtype=torch.float64, device=self.device)
        state = torch.zeros((7, max(q, 1)), dtype=torch.float64, device=self.device)
        panels, have = {}, self.n_pairs > 0

        def init(r, tol):
            panels["R"] = r
            panels["X"], panels["P"], panels["Q"] = (torch.empty_like(r) for _ in range(3))
            self.ctx.check(L.sc_dev_pairs_cg_init_f64(self.ctx.handle, self.n_atoms, self.dim, p(panels["X"]), p(r),
                                                      p(panels["P"]), q, q, float(tol), p(state), p(work), size.value))

            def read():
                host = state.cpu()   # (the synchronisation)
                return host[4].view(torch.int64).numpy().copy(), host[5].view(torch.int64).numpy().copy(), host[0].numpy().copy()

            return panels["X"], read

        def step(iterations):
            self.ctx.check(L.sc_dev_pairs_cg_step_f64(
                self.ctx.handle, p(self._coord), self.n_atoms, self.dim, p(self._pairs) if have else None, self.n_pairs,
                p(self._gamma) if have else None, p(self._row_start), p(self._scale), p(panels["X"]), p(panels["R"]),
                p(panels["P"]), p(panels["Q"]), q, q, p(state), p(work), size.value, int(iterations)))

        return init, step

    def solve(self, f, tol=1e-8, max_iter=2000, check_every=10, deflate=None):
        """
        The minimum-norm solutions ``x = (T H T)^+ f`` by conjugate gradients on the range of the matrix
        (:func:`iterative.conjugate_gradient`, ``csrc/pair_cg.hip``): ``(x, info)``.  ``f`` is (dim n,) or (q, dim n), an array
        or a tensor, rows in the coordinates of the matrix; ``x`` is a CUDA tensor of the same shape.  No (dim n, dim n) matrix
        exists; the right-hand sides run in chunks of at most :attr:`SOLVE_COLUMNS` columns, which bounds the memory.

        The null space -- six rigid-body fields, or the constant vector, each divided by ``t`` -- is projected out of ``f``
        and ``x``; a network of several parts has more zero modes than these, and a right-hand side with a component along
        them does not converge.  A column stops at ``|f_p - H x| <= tol |f_p|``, ``f_p`` the projected right-hand side, which
        bounds its error by ``tol |f_p| / lambda_nz``, ``lambda_nz`` the lowest non-zero eigenvalue.  The status is read on
        the host every ``check_every`` iterations, the only synchronisations; at most ``max_iter`` iterations run.

        ``deflate = (w, v)``: exact eigenpairs as :meth:`lowest_modes` returns them, the trivial rows first; their part of
        the solution is added in closed form and the iteration runs on the rest of the spectrum, condition ``b / w[-1]``
        in place of ``b / lambda_nz``.  What the modes' own residuals leave of ``f_p - H x`` above ``tol |f_p|`` is removed
        by a short second iteration (:func:`iterative.conjugate_gradient`), so the stopping rule holds for computed modes.

        ``info``: ``iterations`` (q,), ``residuals`` (q,) relative to ``|f_p|``, ``status`` (q,) (0 still running, 1
        converged, 2 broken down), ``converged``, ``b``, ``tol``.  Running out of iterations or a breakdown returns what
        there is with ``converged = False``; nothing is raised.  The same arguments give the same bits, and without
        deflation a right-hand side's solution has the same bits alone and in any batch.
        """
        from . import iterative

        shape = tuple(f.shape) if hasattr(f, "shape") else np.shape(f)
        if len(shape) not in (1, 2) or shape[-1] != self.m:
            raise ValueError(f"Expected right-hand sides of shape ({self.m},) or (q, {self.m}), got {shape}")
        tol, max_iter, check_every, deflate = iterative.checked_solve(self.m, tol, max_iter, check_every, deflate)
        torch = self.torch
        rows, single = self._rows(f)   # (every refusal above needs no device)
        b = self.spectral_bound()
        with torch.cuda.device(self.device):
            if deflate is not None:
                deflate = tuple((t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, dtype=np.float64)))
                                .to(device=self.device, dtype=torch.float64) for t in deflate)
            null = self.null_space()
            out = self._empty((len(rows), self.m))
            infos = []
            for lo in range(0, len(rows), self.SOLVE_COLUMNS):
                chunk = rows[lo: lo + self.SOLVE_COLUMNS]
                init, step = self._cg_callables(len(chunk))
                panel = chunk.T.clone(memory_format=torch.contiguous_format)   # (the driver overwrites it)
                x, info = iterative.conjugate_gradient(init, step, panel, null, b, tol=tol, max_iter=max_iter,
                                                       check_every=check_every, deflate=deflate,
                                                       apply=lambda t: self.panel_step(t, torch.empty_like(t), 1.0, 0.0, 0.0))
                out[lo: lo + len(chunk)] = x.T
                infos.append(info)
        info = {key: np.concatenate([i[key] for i in infos]) if infos else np.zeros(0, dtype=kind)
                for key, kind in (("iterations", np.int64), ("residuals", np.float64), ("status", np.int64))}
        info.update(converged=all(i["converged"] for i in infos), b=b, tol=tol)
        return (out[0] if single else out), info

    def linear_response(self, force, atom_scale=None, **solve_options):
        """
        The displacement a force induces (linear response theory, :func:`nma.linear_response`) from the exact pseudo-inverse,
        ``s (T H T)^+ s f`` with ``s`` the operator's own ``t`` repeated per coordinate -- the Cartesian response of a
        mass-weighted network -- or ``atom_scale`` (n,) when given.  ``force`` is (n, 3), (3n,) or (q, n, 3); returns a CUDA
        tensor (n, 3) or (q, n, 3) and the ``info`` of :meth:`solve`, whose options ``solve_options`` are.
        """
        if self.dim != 3:
            raise ValueError("linear_response needs the Hessian, dim 3")
        n = self.n_atoms
        shape = tuple(force.shape) if hasattr(force, "shape") else np.shape(force)
        if shape not in ((n, 3), (3 * n,)) and not (len(shape) == 3 and shape[1:] == (n, 3)):
            raise ValueError(f"Expected a force of shape ({n}, 3), ({3 * n},) or (q, {n}, 3), got {shape}")
        if atom_scale is not None and tuple(np.shape(atom_scale)) != (n,):
            raise IndexError(f"{tuple(np.shape(atom_scale))} scale factors for {n} atoms given")
        from . import iterative

        iterative.checked_solve(self.m, solve_options.get("tol", 1e-8), solve_options.get("max_iter", 2000),
                                solve_options.get("check_every", 10), solve_options.get("deflate"))
        torch = self.torch
        if not isinstance(force, torch.Tensor):
            force = torch.from_numpy(np.ascontiguousarray(force, dtype=np.float64))
        f = force.to(device=self.device, dtype=torch.float64).reshape(-1, 3 * n)
        if atom_scale is None:
            s = self._scale
        elif isinstance(atom_scale, torch.Tensor):
            s = atom_scale.to(device=self.device, dtype=torch.float64)
        else:
            s = torch.from_numpy(np.asarray(atom_scale, dtype=np.float64)).to(self.device)
        s3 = None if s is None else s.repeat_interleave(3)[None, :]
        x, info = self.solve(f if s3 is None else f * s3, **solve_options)
        if s3 is not None:
            x = x * s3
        return (x.reshape(-1, n, 3) if len(shape) == 3 else x.reshape(n, 3)), info

    def covariance_columns(self, atom_index, **solve_options):
        """
        The rows ``dim a .. dim a + dim - 1`` of the pseudo-inverse ``(T H T)^+`` for the listed atoms, a CUDA tensor
        (dim len(atom_index), dim n), and the ``info`` of :meth:`solve`: the exact covariance of these atoms with every atom,
        so their mean-square fluctuations (the traces of the diagonal blocks), their rows of a perturbation response scan
        and their cross-correlations, without the (dim n, dim n) matrix.
        """
        idx = np.asarray(atom_index)
        if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
            raise IndexError("atom_index must be a list of integer atom indices")
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_atoms):
            raise IndexError(f"atom_index holds an atom outside 0..{self.n_atoms - 1}")
        rows = (self.dim * idx.astype(np.int64)[:, None] + np.arange(self.dim)[None, :]).reshape(-1)
        unit = np.zeros((len(rows), self.m))
        unit[np.arange(len(rows)), rows] = 1.0
        return self.solve(unit, **solve_options)
