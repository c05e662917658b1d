"""
Conformational ensembles on the device: least-squares superposition and principal component analysis of M conformations of
the same N atoms (an NMR bundle, a set of crystal structures, MD frames).  The reference has no counterpart -- its callers
superimpose with biotite; Bio3D: ``fit.xyz`` / ``pca.xyz``, ProDy: ``superpose`` / ``iterpose`` / ``PCA``.

:func:`superimpose` is the host convenience for one or a few conformers, e.g. before ``nma.overlap(enm, fitted - fixed)``.
:class:`Ensemble` keeps the frames on the device, fits them on a frame or iteratively on their mean
(``csrc/superpose.hip``), gives the least-squares RMSD of every pair of frames, or which pairs lie within a cutoff as a bit
matrix (``csrc/rmsd_matrix.hip``), and turns them into :class:`EssentialDynamics`, the quasi-harmonic modes of the ensemble
(``csrc/ensemble_pca.hip``): a mode source like :class:`~springcraft_amd.RTB`, with every mode consumer of the batch
solvers and the comparisons ``rmsip`` / ``covariance_overlap`` / ``mode_overlap_matrix`` against an elastic network's modes.
"""

import ctypes as C

import numpy as np

from . import _hip, atoms as _atoms
from .batch import _BatchSolver, _UniformLayout

__all__ = ["Ensemble", "EssentialDynamics", "FrameNeighbours", "superimpose", "rmsd_matrix"]


# ---- host-side argument checks (before any device call) -----------------------------------------------------------------
def _host_frames(coords, what="coords"):
    """(M, N, 3) float64 C-contiguous host array of an ndarray-like ensemble; ValueError for any other shape."""
    a = np.ascontiguousarray(coords, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"Expected {what} with shape (M, N, 3), got {a.shape}")
    if a.shape[0] < 1:
        raise ValueError(f"{what} must hold at least one frame")
    if a.shape[1] < 1:
        raise ValueError(f"{what} must hold at least one atom")
    return a


def _checked_weights(weights, n_atoms):
    """None, or (N,) float64 non-negative finite weights with a positive sum."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n_atoms,):
        raise IndexError(f"{w.shape} weights for {n_atoms} atoms given")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and not negative")
    if not w.sum() > 0:
        raise ValueError("weights must have a positive sum")
    return w


def _checked_masses(masses, n_atoms):
    if masses is None:
        return None
    m = np.ascontiguousarray(masses, dtype=np.float64)
    if m.shape != (n_atoms,):
        raise IndexError(f"{m.shape} masses for {n_atoms} atoms given")
    if not np.all(np.isfinite(m)) or not np.all(m > 0):
        raise ValueError("Masses must be positive and finite")
    return m


def max_components(n_frames, n_atoms):
    """Most principal components an ensemble can give: ``min(M - 1, 3 N - 6)`` (centring and the superposition take the rest)."""
    return max(0, min(int(n_frames) - 1, 3 * int(n_atoms) - 6))


def _checked_n_modes(n_modes, n_frames, n_atoms):
    n_modes = int(n_modes)
    most = max_components(n_frames, n_atoms)
    if not 1 <= n_modes <= most:
        raise ValueError(f"n_modes {n_modes} outside 1..{most}: {n_frames} frames of {n_atoms} atoms have "
                         f"min(M - 1, 3 N - 6) = {most} components")
    return n_modes


def _checked_reference(reference, n_frames, n_atoms):
    """None (iterative), an int frame index in range, or an (N, 3) float64 host array."""
    if reference is None:
        return None
    if isinstance(reference, (int, np.integer)) and not isinstance(reference, bool):
        r = int(reference)
        if not -n_frames <= r < n_frames:
            raise IndexError(f"reference frame {r} is out of bounds for an ensemble of {n_frames} frames")
        return r % n_frames
    ref = np.ascontiguousarray(_atoms.coord(reference) if _atoms.is_atom_array(reference) else reference, dtype=np.float64)
    if ref.shape != (n_atoms, 3):
        raise ValueError(f"Expected a reference of shape ({n_atoms}, 3), got {ref.shape}")
    return ref


def rank_check(variances, n_frames, n_atoms):
    """
    ValueError when a selected variance is not above ``eps * max(M, 3 N) * largest``: what rounding leaves of a zero
    eigenvalue of the product.  ``variances`` descending, host array.
    """
    var = np.asarray(variances, dtype=np.float64)
    if not np.all(np.isfinite(var)):
        raise np.linalg.LinAlgError("the ensemble's variances are not finite: a frame holds a NaN or Inf coordinate")
    floor = np.finfo(np.float64).eps * max(int(n_frames), 3 * int(n_atoms)) * var[0]
    usable = int(np.count_nonzero(var > floor))
    if usable < len(var) or not var[0] > 0:
        raise ValueError(f"the ensemble is rank-deficient: only {usable} of the {len(var)} selected components have a "
                         f"variance above rounding level ({floor:.3e}); ask for n_modes <= {usable}")


_MAX_SIDE = 2 ** 31 - 1


def _checked_matrix_shape(n_a, n_b, n_atoms, workspace_bytes):
    """
    ValueError for an RMSD matrix the kernels cannot index: a side above 2^31 - 1 entries, or sizes for which the library's
    ``sc_rmsd_matrix_workspace`` (``workspace_bytes(n_a, n_b or 0, n_atoms)``) answers -1.  ``n_b`` None: self-comparison.
    """
    n_a, n_atoms = int(n_a), int(n_atoms)
    side_b = n_a if n_b is None else int(n_b)
    if n_a > _MAX_SIDE or side_b > _MAX_SIDE:
        raise ValueError(f"an RMSD matrix of {n_a} x {side_b} frames has more than 2^31 - 1 entries per side")
    if workspace_bytes(n_a, 0 if n_b is None else side_b, n_atoms) < 0:
        raise ValueError(f"an RMSD matrix of {n_a} x {side_b} frames of {n_atoms} atoms is beyond the kernels' index range")
    return n_a, side_b


def _same_weights(a, b):
    """Whether two ensembles' host weights (None or (N,) arrays) are the same."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _upload(torch, host, device):
    """A host array as a tensor on ``device`` (torch wraps writable arrays only: a read-only one is copied first)."""
    return torch.from_numpy(host if host.flags.writeable else host.copy()).to(device)


class EssentialDynamics(_BatchSolver):
    """
    The principal components of a fitted ensemble as a mode set, a batch of one built like :class:`~springcraft_amd.RTB`.
    Made by :meth:`Ensemble.pca`, not directly.

    ``v`` (1, k, 3N): the components, unit rows by descending variance.  ``w`` (1, k) = 1 / variance, ascending: the
    eigenvalues of the quasi-harmonic Hessian in units of kT.  Row r is global mode ``6 + r``, as for an ANM solved with
    ``subset_by_index=(6, 5 + k)``: the six rigid-body modes a superposed ensemble does not have are not stored, and
    ``mode_subset`` counts from 6.  ``variances`` (k,), ``total_variance`` (0-dim) and ``explained_variance_ratio`` (k,) are
    CUDA tensors.  With ``masses`` the components live in mass-weighted coordinates and ``inv_sqrt_mass`` (1, N) is set, for
    the consumers' ``atom_scale=``.

    Every mode consumer of the batch solvers works, with a leading batch axis of one: ``mean_square_fluctuation`` (kT = 1:
    the ensemble's MSF within the k components), ``bfactor``, ``dcc`` (the ensemble's cross-correlation),
    ``anisotropic_fluctuation``, ``overlap``, ``collectivity``, ``distance_fluctuation``, ``linear_response``,
    ``mode_displacement``, ``prs``; and ``rmsip`` / ``covariance_overlap`` / ``mode_overlap_matrix`` with ``other=`` a
    :class:`~springcraft_amd.batch.DeviceBatchSolver` or :class:`~springcraft_amd.RTB` of the same ``n_atoms``, device and
    stream: the comparison of an elastic network with the ensemble.

    Everything is enqueued; :meth:`finish` waits and raises ValueError for a rank-deficient ensemble.
    """

    def __init__(self, ensemble, n_modes, masses):
        ens = ensemble
        self.torch, self.device, self._L, self.ctx, self._stream = ens.torch, ens.device, ens._L, ens.ctx, ens._stream
        self.n_atoms, self.n_frames = ens.n_atoms, ens.n_frames
        k = int(n_modes)
        self.batch, self.dim, self.m = 1, 3, 3 * self.n_atoms
        self.window, self.max_modes, self.counts = None, None, None
        self.subset, self.nvec = (6, 5 + k), k
        self._first_row, self._common_modes = 6, self.m
        self._layout = _UniformLayout(1, self.n_atoms, 3)
        self.masses = masses
        torch = self.torch
        with torch.cuda.device(self.device):
            self.w = self._empty((1, k))
            self.v = self._empty((1, k, self.m))
            self.variances = self._empty((k,))
            self.total_variance = self._empty(())
            sqrt_mass = None if masses is None else torch.from_numpy(np.sqrt(masses)).to(self.device)
            self.inv_sqrt_mass = None if masses is None else (1.0 / sqrt_mass)[None, :].contiguous()
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
            mean = ens.mean()
            self.ctx.check(self._L.sc_dev_ensemble_pca_f64(
                self.ctx.handle, p(ens.frames), self.n_frames, self.n_atoms, p(mean), p(sqrt_mass), k, p(self.w),
                p(self.variances), p(self.v), p(self.total_variance)))
            self._keep = (sqrt_mass, mean)     # (inputs of the enqueued call)

    @property
    def explained_variance_ratio(self):
        """(k,) CUDA tensor ``variances / total_variance``."""
        return self.variances / self.total_variance

    def finish(self):
        """
        Waits for what was enqueued and raises what only the device could find out: ``np.linalg.LinAlgError`` for a
        non-finite frame, ValueError when a selected variance is not above ``eps * max(M, 3N) * largest variance`` -- the
        ensemble is rank-deficient; the message names how many components were usable.  Returns (w, v).
        """
        self.ctx.synchronize()
        rank_check(self.variances.cpu().numpy(), self.n_frames, self.n_atoms)
        return self.w, self.v


class FrameNeighbours:
    """
    What :meth:`Ensemble.neighbours` returns, CUDA tensors: ``bits`` (M, ceil(M / 64)) int64, bit ``g & 63`` of word
    ``g >> 6`` of row f set when frames f and g are neighbours (equal to its transpose; the bits of the columns >= M of the
    last word are 0); ``counts`` (M,) int32, the rows' popcounts: a frame's number of neighbours, itself included, 0 for a
    non-finite frame; ``valid`` (ceil(M / 64),) int64, the bit set of the finite frames.  ``n_frames`` and ``cutoff`` as given.
    """

    def __init__(self, torch, n_frames, cutoff, bits, counts, valid):
        self.torch, self.n_frames, self.cutoff = torch, n_frames, cutoff
        self.bits, self.counts, self.valid = bits, counts, valid

    def dense(self):
        """(M, M) bool CUDA tensor of the bits, for inspection: M^2 bytes.  Only enqueues."""
        torch = self.torch
        shifts = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        return ((self.bits[:, :, None] >> shifts) & 1).bool().reshape(self.n_frames, -1)[:, : self.n_frames]


class Ensemble:
    """
    M conformations of the same N atoms on the device.

    Parameters
    ----------
    coords : ndarray or CUDA float64 tensor, shape=(M, N, 3)
        The ensemble keeps its own copy: superposition moves the copy, never the caller's data.
    weights : ndarray, shape=(N,), optional
        Atom weights of the superposition and of :meth:`rmsd`, non-negative with a positive sum (a zero leaves an atom out
        of the fit; it is still moved with its frame).
    device : int, optional

    ``frames`` is the (M, N, 3) CUDA tensor of the frames as they are now.  All work is enqueued on torch's current stream.
    """

    def __init__(self, coords, weights=None, device=None):
        is_tensor = type(coords).__module__.split(".")[0] == "torch"
        if is_tensor:
            if not coords.is_cuda or str(coords.dtype) != "torch.float64":
                raise ValueError("coords must be an ndarray or a CUDA float64 tensor of shape (M, N, 3)")
            if coords.ndim != 3 or coords.shape[2] != 3:
                raise ValueError(f"Expected coords with shape (M, N, 3), got {tuple(coords.shape)}")
            if coords.shape[0] < 1 or coords.shape[1] < 1:
                raise ValueError("coords must hold at least one frame and one atom")
            if device is not None and coords.device.index != int(device):
                raise ValueError(f"coords is on {coords.device}, the ensemble was asked for device {int(device)}")
            host = None
            shape = tuple(coords.shape)
        else:
            host = _host_frames(coords)
            shape = host.shape
        self.n_frames, self.n_atoms = int(shape[0]), int(shape[1])
        w = _checked_weights(weights, self.n_atoms)
        self.weights = w

        import torch

        self.torch = torch
        if is_tensor:
            self.device = coords.device
        else:
            self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self._L = _hip.lib()
        self._stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx = _hip.Context(self.device.index, stream=self._stream)
        with torch.cuda.device(self.device):
            self.frames = coords.contiguous().clone() if is_tensor else _upload(torch, host, self.device)
            self._w = None if w is None else _upload(torch, w, self.device)
        self._mean = self._msd = None
        self.fit_rmsd = None    # (M,) RMSD of every frame to the target of the last superposition pass

    def _empty(self, shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.device)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _fit(self, target, out, rmsd, rot=None, trans=None):
        p = self._p
        self.ctx.check(self._L.sc_dev_superpose_f64(self.ctx.handle, p(self.frames), self.n_frames, self.n_atoms, p(target),
                                                    p(self._w), p(out), p(rot), p(trans), p(rmsd)))

    def _moments(self):
        if self._mean is None:
            with self.torch.cuda.device(self.device):
                self._mean, self._msd = self._empty((self.n_atoms, 3)), self._empty((self.n_atoms,))
                p = self._p
                self.ctx.check(self._L.sc_dev_ensemble_mean_f64(self.ctx.handle, p(self.frames), self.n_frames,
                                                                self.n_atoms, None, p(self._mean), p(self._msd)))
        return self._mean, self._msd

    # ---- superposition ---------------------------------------------------------------------------------------------------
    def superpose(self, reference=None, tol=1e-4, max_iter=50):
        """
        Fits every frame on a target, in place, with the ensemble's atom weights.

        reference : int, an (N, 3) array / AtomArray, or None
            A frame index or a structure: one pass.  None: iterative fitting on the running mean (ProDy's ``iterpose``):
            the frames are fitted on frame 0, then on their mean, until the RMSD between two successive means is below
            ``tol`` (1e-4 Angstrom is ProDy's default) or ``max_iter`` passes were made.  One scalar is read per pass.

        Returns ``(passes, converged)``; running out of passes does not raise.  ``fit_rmsd`` (M,) holds every frame's RMSD
        to the last target.
        """
        ref = _checked_reference(reference, self.n_frames, self.n_atoms)
        tol, max_iter = float(tol), int(max_iter)
        if reference is None and (not tol > 0 or max_iter < 1):
            raise ValueError("tol must be positive and max_iter at least 1")
        torch = self.torch
        with torch.cuda.device(self.device):
            rmsd = self._empty((self.n_frames,))
            if ref is not None:
                target = self.frames[ref].clone() if isinstance(ref, int) else _upload(torch, ref, self.device)
                self._fit(target, self.frames, rmsd)
                self._mean = self._msd = None
                self.fit_rmsd = rmsd
                return 1, True
            target = self.frames[0].clone()
            passes, converged = 0, False
            while passes < max_iter:
                self._fit(target, self.frames, rmsd)
                passes += 1
                self._mean = self._msd = None
                mean = self._moments()[0]
                step = float(torch.sqrt(((mean - target) ** 2).sum(dim=1).mean()))   # (the pass's one host read)
                target = mean
                if step < tol:
                    converged = True
                    break
            self.fit_rmsd = rmsd
            return passes, converged

    # ---- what the fitted frames say -----------------------------------------------------------------------------------------
    def mean(self):
        """(N, 3) CUDA tensor, the mean frame (a fixed-order sum: two calls agree bit for bit).  Only enqueues."""
        return self._moments()[0]

    def rmsf(self):
        """
        (N,) CUDA tensor ``sqrt(sum_f |x_f[a] - mean[a]|^2 / (M - 1))``, the root mean square fluctuation of every atom
        about the mean frame with the sample normaliser of :meth:`pca`'s covariance (0 for one frame): ``rmsf() ** 2`` is
        what ``pca(M - 1).mean_square_fluctuation()`` gives.
        """
        msd = self._moments()[1]
        m = self.n_frames
        return self.torch.sqrt(msd * (m / (m - 1.0) if m > 1 else 0.0))

    def rmsd(self, reference=None):
        """
        (M,) CUDA tensor: every frame's weighted least-squares RMSD to the mean frame (None), to frame ``reference`` or to
        an (N, 3) structure.  The frames are fitted in a temporary; the ensemble is not moved.
        """
        ref = _checked_reference(reference, self.n_frames, self.n_atoms)
        torch = self.torch
        with torch.cuda.device(self.device):
            if ref is None:
                target = self.mean()
            else:
                target = self.frames[ref].clone() if isinstance(ref, int) else _upload(torch, ref, self.device)
            out, rmsd = self._empty(tuple(self.frames.shape)), self._empty((self.n_frames,))
            self._fit(target, out, rmsd)
            return rmsd

    # ---- frame against frame ------------------------------------------------------------------------------------------------
    def _checked_other(self, other):
        if other is None:
            return None
        if not isinstance(other, Ensemble):
            raise ValueError(f"other must be an Ensemble, got {type(other).__name__}")
        if other.n_atoms != self.n_atoms:
            raise ValueError(f"other has {other.n_atoms} atoms, this ensemble {self.n_atoms}")
        if not _same_weights(self.weights, other.weights):
            raise ValueError("other must have the same atom weights as this ensemble")
        if other.device != self.device:
            raise ValueError(f"other is on {other.device}, this ensemble on {self.device}")
        return other

    def rmsd_matrix(self, other=None, fit=True, squared=False):
        """
        (M, M) CUDA tensor, the weighted RMSD of every pair of frames after the least-squares superposition of the pair
        (``fit=False``: of the frames as they are); with ``other``, an :class:`Ensemble` of the same atoms, weights and
        device, (M, other.n_frames).  ``squared``: the mean-square deviation.  One Gram product over the atoms gives the
        3 x 3 cross-covariance of every pair, and the RMSD follows from its Horn matrix's largest eigenvalue: no frame is
        rotated or written, the ensemble is not moved.  The rotation is proper also for a mirror image.

        The self-comparison equals its transpose bit for bit and has an exactly zero diagonal; a frame with a non-finite
        coordinate gives a NaN row and column (its diagonal entry too) and nothing else; an entry's bits depend on its two
        frames and the weights alone.  Only enqueues.
        """
        other = self._checked_other(other)
        n_a, n_b = _checked_matrix_shape(self.n_frames, None if other is None else other.n_frames, self.n_atoms,
                                         self._L.sc_rmsd_matrix_workspace)
        p = self._p
        with self.torch.cuda.device(self.device):
            out = self._empty((n_a, n_b))
            self.ctx.check(self._L.sc_dev_rmsd_matrix_f64(
                self.ctx.handle, p(self.frames), n_a, None if other is None else p(other.frames), n_b, self.n_atoms,
                p(self._w), (1 if fit else 0) | (2 if squared else 0), p(out)))
        return out

    def medoid(self, fit=True):
        """
        0-dim CUDA integer tensor: the index of the frame with the smallest sum of squared RMSD to all other frames, the
        first one among equals; frames with a non-finite coordinate neither count nor are counted.  Computed with torch
        from ``rmsd_matrix(squared=True)``; nothing is read back.  (All frames non-finite: 0.)
        """
        torch = self.torch
        msd = self.rmsd_matrix(fit=fit, squared=True)
        bad = torch.isnan(torch.diagonal(msd))
        total = torch.where(bad[None, :], torch.zeros_like(msd), msd).sum(dim=1)
        total = torch.where(bad, torch.full_like(total, float("inf")), total)
        # the first index of the minimum (argmin's choice among equals is not specified)
        index = torch.arange(self.n_frames, device=self.device)
        return torch.where(total == total.min(), index, torch.full_like(index, self.n_frames)).min().clamp(max=self.n_frames - 1)

    def neighbours(self, cutoff, fit=True, squared=False):
        """
        :class:`FrameNeighbours`: which frames lie within ``cutoff`` of which, ``rmsd_matrix(fit=fit, squared=squared) <=
        cutoff`` as an (M, ceil(M / 64)) bit matrix and its row counts, written by the product kernel of the matrix without
        the matrix: M^2 / 8 bytes, not 8 M^2.  A bit is the comparison of exactly the value ``rmsd_matrix`` would hold.  A
        frame is its own neighbour; a frame with a non-finite coordinate has no neighbours and is nobody's.  The counts are
        a density per frame, the bits a contact graph of conformers, and what ``cluster(matrix_free=True)`` runs on.
        ValueError for a cutoff that is negative or not finite and for more than ``cluster.MAX_ITEMS`` frames.  Only enqueues.
        """
        from . import cluster as _cluster

        cut = _cluster.check_gromos_args(self.n_frames, cutoff, None, 1)[0]
        _cluster.check_frame_counts(self.n_frames, self.n_atoms)
        torch, n = self.torch, self.n_frames
        words = (n + 63) // 64
        p = self._p
        with torch.cuda.device(self.device):
            bits = torch.empty((n, words), dtype=torch.int64, device=self.device)
            counts = torch.empty((n,), dtype=torch.int32, device=self.device)
            valid = torch.empty((words,), dtype=torch.int64, device=self.device)
            self.ctx.check(self._L.sc_dev_frame_neighbours_f64(
                self.ctx.handle, p(self.frames), n, self.n_atoms, p(self._w), (1 if fit else 0) | (2 if squared else 0), cut,
                p(bits), p(counts), p(valid)))
        return FrameNeighbours(torch, n, cut, bits, counts, valid)

    def cluster(self, method="gromos", cutoff=None, k=None, fit=True, squared=False, matrix_free=False, **options):
        """
        The frames put into clusters by their pairwise RMSD: a :class:`~springcraft_amd.cluster.Clustering` of CUDA
        tensors from ``rmsd_matrix(fit=fit, squared=squared)``, which is handed to the kernels where it is, not copied.
        ``method="gromos"`` with ``cutoff`` (in the matrix' units: squared with ``squared``) is
        :func:`~springcraft_amd.cluster.cluster_gromos`, ``method="kmedoids"`` with ``k``
        :func:`~springcraft_amd.cluster.cluster_kmedoids`; ``options`` go to them (``max_clusters``, ``max_iter``,
        ``check_every``).  A frame with a non-finite coordinate gets label -1.  ``k=1, squared=True`` gives :meth:`medoid`.
        ``matrix_free=True`` (``"gromos"`` only: k-medoids reads the matrix in every pass) never stores the matrix: the
        product kernel writes the neighbour bits of :meth:`neighbours` into the run's workspace and the same rounds follow,
        with the same result in 1 / 64 of the memory.
        ValueError before any device work for an unknown method, a method without its parameter or a parameter out of range.
        """
        from . import cluster as _cluster

        if matrix_free and method == "kmedoids":
            raise ValueError("matrix_free is for method 'gromos': k-medoids reads the matrix in every pass")
        if method == "gromos":
            if k is not None:
                raise ValueError("method 'gromos' takes a cutoff, not k")
            _cluster.check_gromos_args(self.n_frames, cutoff, options.get("max_clusters"), options.get("check_every", 32))
        elif method == "kmedoids":
            if cutoff is not None:
                raise ValueError("method 'kmedoids' takes k, not a cutoff")
            _cluster.check_kmedoids_args(self.n_frames, k, options.get("max_iter", 100), options.get("check_every", 4))
        else:
            raise ValueError(f"method must be 'gromos' or 'kmedoids', got {method!r}")
        unknown = set(options) - ({"max_clusters", "check_every"} if method == "gromos" else {"max_iter", "check_every"})
        if unknown:
            raise ValueError(f"method {method!r} does not take {sorted(unknown)}")
        _cluster.workspace_bytes(self.n_frames, 0 if method == "gromos" else int(k))
        if matrix_free:
            return _cluster.gromos_from_frames(self, cutoff, fit=fit, squared=squared, **options)
        dist = self.rmsd_matrix(fit=fit, squared=squared)
        if method == "gromos":
            return _cluster.cluster_gromos(dist, cutoff, **options)
        return _cluster.cluster_kmedoids(dist, k, **options)

    def deviations(self):
        """(M, N, 3) CUDA tensor, every frame minus the mean frame: displacement vectors for ``overlap()``."""
        return (self.frames - self.mean()[None, :, :]).contiguous()

    def pca(self, n_modes=20, masses=None):
        """
        The ``n_modes`` largest principal components of the frames as they are (fit them first) about their mean, as
        :class:`EssentialDynamics`; ``masses`` (N,): mass-weighted (quasi-harmonic) coordinates.  ``n_modes`` above
        ``min(M - 1, 3N - 6)`` raises ValueError.  Only enqueues.
        """
        k = _checked_n_modes(n_modes, self.n_frames, self.n_atoms)
        return EssentialDynamics(self, k, _checked_masses(masses, self.n_atoms))


def superimpose(fixed, mobile, weights=None, return_transform=False, device=None):
    """
    Least-squares superposition of ``mobile`` on ``fixed`` on the device, host arrays in and out.

    fixed : ndarray (N, 3) or AtomArray
    mobile : ndarray (N, 3) or (M, N, 3), or AtomArray
    weights : ndarray (N,), optional

    Returns ``(fitted, rmsd)``: ``fitted`` with the shape of ``mobile``, ``rmsd`` a float or (M,); with
    ``return_transform`` also ``(R, t)``, (3, 3) and (3,) or (M, 3, 3) and (M, 3), with ``fitted = mobile @ R.T + t``.
    The rotations are proper (det = +1) also for a mirror image.  Use it before ``nma.overlap(enm, fitted - fixed)``.
    """
    fix = np.ascontiguousarray(_atoms.coord(fixed) if _atoms.is_atom_array(fixed) else fixed, dtype=np.float64)
    if fix.ndim != 2 or fix.shape[1] != 3:
        raise ValueError(f"Expected fixed coordinates with shape (N, 3), got {fix.shape}")
    mob = np.asarray(_atoms.coord(mobile) if _atoms.is_atom_array(mobile) else mobile, dtype=np.float64)
    single = mob.ndim == 2
    mob = _host_frames(mob[None] if single else mob, "mobile")
    if mob.shape[1:] != fix.shape:
        raise ValueError(f"mobile has {mob.shape[1]} atoms, fixed {fix.shape[0]}")
    ens = Ensemble(mob, weights=weights, device=device)
    torch = ens.torch
    with torch.cuda.device(ens.device):
        target = _upload(torch, fix, ens.device)
        rmsd, rot, trans = ens._empty((ens.n_frames,)), ens._empty((ens.n_frames, 3, 3)), ens._empty((ens.n_frames, 3))
        ens._fit(target, ens.frames, rmsd, rot, trans)
        ens.ctx.synchronize()
        fitted, rmsd, rot, trans = (t.cpu().numpy() for t in (ens.frames, rmsd, rot, trans))
    if single:
        fitted, rmsd, rot, trans = fitted[0], float(rmsd[0]), rot[0], trans[0]
    return (fitted, rmsd, (rot, trans)) if return_transform else (fitted, rmsd)


def rmsd_matrix(coords, other=None, weights=None, fit=True, squared=False, device=None):
    """
    The pairwise RMSD matrix of host arrays on the device, like :func:`superimpose`: ``coords`` (M, N, 3) against itself, or
    against ``other`` (K, N, 3).  Returns an (M, M) or (M, K) ndarray; see :meth:`Ensemble.rmsd_matrix`.
    """
    a = _host_frames(coords)
    b = None if other is None else _host_frames(other, "other")
    if b is not None and b.shape[1] != a.shape[1]:
        raise ValueError(f"other has {b.shape[1]} atoms, coords {a.shape[1]}")
    w = _checked_weights(weights, a.shape[1])
    ens = Ensemble(a, weights=w, device=device)
    out = ens.rmsd_matrix(None if b is None else Ensemble(b, weights=w, device=ens.device.index), fit=fit, squared=squared)
    ens.ctx.synchronize()
    return out.cpu().numpy()
