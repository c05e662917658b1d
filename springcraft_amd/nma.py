"""
Normal-mode analysis on top of the device eigensolver.

``eigen`` is the hot-path function (reference: nma.py:29-63): a dense symmetric float64
eigendecomposition, here performed by the hand-written HIP solver (``csrc/eigh*.hip``) instead
of LAPACK ``dsyevd``.  The mode-subset consumers (``frequencies``, ``mean_square_fluctuation``,
``bfactor``, ``dcc``, ``prs``; reference: nma.py:66-359, :476-524) run on the device-resident
eigenpairs: the (n, n) eigenvector matrix never crosses PCIe for them.  ``mean_square_fluctuation``, ``bfactor``, ``dcc``
and ``anisotropic_fluctuation`` (no reference counterpart: the per-atom 3x3 tensors whose trace is the MSF) are the batch
kernels of ``csrc/batch_consumers.hip`` with a batch of one, ``prs`` is ``csrc/consumers.hip``; ``anisotropy`` reduces the
tensors on the host.
``overlap`` and ``collectivity`` (no reference counterpart: which modes carry a displacement, and how many atoms a mode
moves) are one pass along the selected rows (``csrc/mode_overlap.hip``); ``cumulative_overlap`` is array arithmetic.
``distance_fluctuation`` (no reference counterpart: how much every inter-atom distance fluctuates) is the pair kernel of
``csrc/dist_fluct.hip`` with a batch of one; ``effective_stiffness`` is array arithmetic on its result.
``linear_response`` (reference: nma.py:422-473) and ``mode_displacement`` (no reference counterpart: a displacement field
built from chosen modes) are the two passes of ``csrc/mode_response.hip`` over the selected rows, in mode space: no
covariance is formed and only (q, 3N) numbers cross PCIe; ``sample_displacements`` draws the coefficients on the host.
``deformation_energy`` and ``spring_strain`` (no reference counterpart: where a mode strains the network) run the selected
modes through the pair-list operator of ``csrc/pair_operator.hip`` (:class:`~springcraft_amd.PairOperator`).
``rmsip``, ``covariance_overlap`` and ``mode_overlap_matrix`` (no reference counterpart: how the modes of one model compare
with those of another) run the pair kernel of ``csrc/mode_subspace.hip`` on the two models' device-resident eigenpairs.
``normal_mode`` and ``effector_sensor`` are O(n) / O(n^2) host arithmetic on results that are already on the host.
"""


import numpy as np

from . import _hip

__all__ = [
    "eigen", "eigh", "pinvh", "frequencies", "mean_square_fluctuation", "bfactor", "dcc",
    "normal_mode", "linear_response", "prs", "effector_sensor", "anisotropic_fluctuation", "anisotropy",
    "overlap", "collectivity", "cumulative_overlap", "distance_fluctuation", "effective_stiffness",
    "mode_displacement", "sample_displacements", "deformation_energy", "spring_strain",
    "rmsip", "covariance_overlap", "mode_overlap_matrix", "generalized_correlation",
]

K_B = 1.380649e-23
N_A = 6.02214076e23


def _value_window(subset_by_value, subset_by_index=None):
    """
    ``subset_by_value`` checked as ``scipy.linalg.eigh`` checks it (same errors, before any device call): None, or the
    bounds (vl, vu) as floats, vl < vu, +-inf allowed.
    """
    if subset_by_value is None:
        return None
    if subset_by_index is not None:
        raise ValueError("Either index or value subset can be requested.")
    vl, vu = (float(x) for x in subset_by_value)
    if not (vl < vu):   # (also a NaN bound)
        raise ValueError("Requested eigenvalue bounds are not valid. Valid range is (-inf, inf) and low < high, but "
                         f"low={vl}, high={vu} is given")
    return vl, vu


def eigh(matrix, eigenvectors=True, subset_by_index=None, subset_by_value=None):
    """
    Device replacement for ``np.linalg.eigh(matrix)`` as used at nma.py:61: ascending
    eigenvalues of a symmetric float64 matrix (lower triangle read) and, as ROWS, the
    corresponding eigenvectors (``eig_vectors[i]`` belongs to ``eig_values[i]``).

    ``subset_by_index=(lo, hi)`` (inclusive, like ``scipy.linalg.eigh``) selects the partial-spectrum
    path: only eigenpairs lo..hi are computed (bisection + inverse iteration), which is what large
    models that only need their slowest modes should use.

    ``subset_by_value=(vl, vu)`` (like ``scipy.linalg.eigh``) selects the eigenvalues in the half-open interval
    (vl, vu], +-inf allowed: the m of them are counted on the device on the tridiagonal matrix that is then solved (one
    tridiagonalisation), and exactly m pairs are returned, ``w`` (m,) and ``v`` (m, n); m may be 0.  Whether an eigenvalue
    within about n eps ||A|| of a bound is inside is decided by that count, as LAPACK's dsyevr decides it.  For an ENM,
    eigenvalue and frequency are related by lambda = (2 pi f)^2 (:func:`frequencies`); the six trivial eigenvalues of an
    ANM sit at rounding level around zero (|lambda| ~ 1e-14 .. 1e-13 of lambda_max, either sign), so a window meant to
    skip them needs a small positive ``vl``.  Giving both subsets, ``vl >= vu`` or a NaN bound raises ValueError.
    """
    window = _value_window(subset_by_value, subset_by_index)
    a = np.ascontiguousarray(matrix, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"Expected a square matrix, got shape {a.shape}")
    n = a.shape[0]
    ctx = _hip.context()
    if window is not None:
        w, v = _hip.solve_window(ctx, _hip.lib().sc_eigh_window_f64, (ctx.handle, _hip.ptr(a), n) + window, n,
                                 eigenvectors)
        return (w, v) if eigenvectors else w
    if subset_by_index is not None:
        lo, hi = (int(x) for x in subset_by_index)
        if not (0 <= lo <= hi < n):
            raise ValueError(f"subset_by_index {subset_by_index} out of range for order {n}")
        m = hi - lo + 1
        w = np.empty(m, dtype=np.float64)
        v = np.empty((m, n), dtype=np.float64) if eigenvectors else None
        ctx.check(_hip.lib().sc_eigh_range_f64(ctx.handle, _hip.ptr(a), n, lo, hi, _hip.ptr(w), _hip.ptr(v)))
        return (w, v) if eigenvectors else w
    w = np.empty(n, dtype=np.float64)
    v = _hip.host_array((n, n)) if eigenvectors else None
    ctx.check(_hip.lib().sc_eigh_f64(ctx.handle, _hip.ptr(a), n, _hip.ptr(w), _hip.ptr(v)))
    return (w, v) if eigenvectors else w


def pinvh(matrix, rcond=1e-6):
    """
    Device replacement for ``np.linalg.pinv(matrix, hermitian=True, rcond=rcond)`` as used by the
    ``covariance`` / ``hessian`` / ``kirchhoff`` properties (anm.py:114-117,132-136; gnm.py:107-110,125-131).
    """
    a = np.ascontiguousarray(matrix, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"Expected a square matrix, got shape {a.shape}")
    n = a.shape[0]
    out = _hip.host_array((n, n))
    ctx = _hip.context()
    ctx.check(_hip.lib().sc_pinvh_f64(ctx.handle, _hip.ptr(a), n, float(rcond), _hip.ptr(out)))
    return out


def _model_kind(enm):
    from .anm import ANM
    from .gnm import GNM

    if isinstance(enm, GNM):
        return "gnm", 1
    if isinstance(enm, ANM):
        return "anm", 6
    raise ValueError("Instance of GNM/ANM class expected.")


def eigen(enm, subset_by_index=None, subset_by_value=None):
    """
    Eigenvalues (ascending) and eigenvectors (rows) of the Kirchhoff / Hessian matrix of a
    GNM / ANM (reference: nma.py:29-63).  ``subset_by_index=(lo, hi)`` (extension, inclusive) restricts
    the computation to modes lo..hi; ``subset_by_value=(vl, vu)`` (extension, scipy's semantics, see :func:`eigh`) to the
    modes whose eigenvalue lies in (vl, vu].  lambda = (2 pi f)^2: every mode below the frequency f is
    ``subset_by_value=(vl, (2 * np.pi * f) ** 2)``.  An ANM's six trivial eigenvalues are ~0 at rounding level, of either
    sign (|lambda| ~ 1e-14 .. 1e-13 of lambda_max): ``vl = -inf`` includes them, a small positive ``vl`` (e.g. 1e-6
    lambda_max) leaves them out.
    """
    _model_kind(enm)
    _value_window(subset_by_value, subset_by_index)
    return enm._eigen_device(subset_by_index, subset_by_value)


def frequencies(enm):
    """Frequencies sqrt(lambda)/(2 pi) of all modes; trivial eigenvalues enter as |lambda| (nma.py:66-105)."""
    _, ntriv = _model_kind(enm)
    w = enm._modes_device().values()
    w[:ntriv] = np.abs(w[:ntriv])
    return np.sqrt(w) / (2 * np.pi)


def _mode_selection(enm, mode_subset, n_modes):
    _, ntriv = _model_kind(enm)
    if mode_subset is None:
        return np.arange(ntriv, n_modes)
    subset = np.asarray(mode_subset)
    if np.any(subset < ntriv):
        raise ValueError("Trivial modes are included in the current selection. Please check your input.")
    return subset


def mean_square_fluctuation(enm, mode_subset=None, tem=None, tem_factors=K_B):
    """Per-atom mean square fluctuation sum_k v_k^2 / lambda_k over the selected modes (nma.py:108-184)."""
    _model_kind(enm)
    modes = enm._modes_device()
    contrib = modes.msf(_mode_selection(enm, mode_subset, modes.order))
    if tem is not None:
        contrib = contrib * (tem * tem_factors)
    return contrib


def bfactor(enm, mode_subset=None, tem=None, tem_factors=K_B):
    """Isotropic B-factors 8 pi^2/3 x MSF (nma.py:187-230)."""
    return (8 * np.pi**2) / 3 * mean_square_fluctuation(enm, mode_subset, tem, tem_factors)


def dcc(enm, mode_subset=None, norm=True, tem=None, tem_factors=K_B):
    """Dynamic cross-correlation between nodes over the selected modes (nma.py:233-359)."""
    _model_kind(enm)
    modes = enm._modes_device()
    if mode_subset is None:
        # all modes: the reference takes the covariance matrix here (nma.py:324-336), i.e. pinv(M, hermitian=True,
        # rcond=1e-6): every mode with |lambda| > 1e-6 max|lambda| -- which drops the trivial modes and, on a nearly
        # disconnected network, also non-trivial modes below that threshold
        w = modes.values()
        sel = np.nonzero(np.abs(w) > 1e-6 * np.abs(w).max())[0]
    else:
        sel = _mode_selection(enm, mode_subset, modes.order)
    # sum_k <v_k[a], v_k[b]> / lambda_k, normalised by sqrt(c_aa c_bb) on request
    cov = modes.dcc(sel, norm)
    if tem is not None:  # applied after the normalisation, as the reference does (nma.py:355-357)
        cov = cov * tem * tem_factors
    return cov


# position of tensor entry (d, e) among the six stored values xx yy zz xy xz yz, the order of a PDB ANISOU record
ANISOU_INDEX = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])


def _aniso_full(u6):
    """(..., 6) values in ANISOU order -> (..., 3, 3) symmetric tensors (an index gather; works on NumPy arrays)."""
    return u6[..., ANISOU_INDEX]


def anisotropic_fluctuation(anm, mode_subset=None, tem=None, tem_factors=K_B):
    """
    Per-atom anisotropic fluctuation tensors ``U[a] = sum_k v_k[a] v_k[a]^T / lambda_k`` over the selected modes, shape
    (n, 3, 3), symmetric: the anisotropic displacement parameters one compares with ANISOU records, i.e. the diagonal
    3x3 blocks of the covariance restricted to the selection.  ``trace(U[a])`` is :func:`mean_square_fluctuation` of
    the same selection, whose ``mode_subset`` (None: every non-trivial mode), ``tem`` and ``tem_factors`` this takes.
    The reference has no counterpart; there one forms ``anm.covariance`` and reads its blocks.  Here it is one pass
    over the selected device-resident eigenvectors.  ANM only.
    """
    from .anm import ANM

    if not isinstance(anm, ANM):
        raise ValueError("Instance of ANM class expected.")
    if mode_subset is not None:
        mode_subset = _mode_selection(anm, mode_subset, None)   # (the trivial-mode error needs no device)
    modes = anm._modes_device()
    if mode_subset is None:
        mode_subset = _mode_selection(anm, None, modes.order)
    tensors = _aniso_full(modes.aniso(mode_subset))
    if tem is not None:
        tensors = tensors * (tem * tem_factors)
    return tensors


def anisotropy(tensors):
    """
    Smallest over largest eigenvalue of each 3x3 tensor of ``tensors`` (..., n, 3, 3) -> (..., n): 1 for an isotropic
    atom, towards 0 for motion confined to a plane or a line (the figure ANISOU validation reports).  NaN where the largest
    eigenvalue is 0 (an empty selection) or the tensor is not finite.  Host NumPy on a result that is already there.
    """
    t = np.asarray(tensors, dtype=np.float64)
    if t.shape[-2:] != (3, 3):
        raise ValueError(f"Expected tensors of shape (..., 3, 3), got {t.shape}")
    finite = np.isfinite(t).all(axis=(-2, -1))
    lam = np.linalg.eigvalsh(np.where(finite[..., None, None], t, 0.0))
    ok = finite & (lam[..., 2] != 0)
    out = np.full(lam.shape[:-1], np.nan)
    np.divide(lam[..., 0], lam[..., 2], out=out, where=ok)
    return out


def _displacement(enm, displacement):
    """``displacement`` as a C-contiguous float64 (q, dim * N) array, and whether the caller gave a single vector."""
    kind, _ = _model_kind(enm)
    n = len(enm._coord)
    tail = (n, 3) if kind == "anm" else (n,)
    d = np.asarray(displacement, dtype=np.float64)
    if d.shape != tail and d.shape[1:] != tail:
        names = "(N, 3) or (q, N, 3)" if kind == "anm" else "(N,) or (q, N)"
        raise ValueError(f"Expected a displacement of shape {names} with N = {n} for this {kind.upper()}, got {d.shape}")
    single = d.shape == tail
    return np.ascontiguousarray(d.reshape(1 if single else d.shape[0], -1)), single


def overlap(enm, displacement, mode_subset=None):
    """
    Overlap of the selected modes with a displacement, ``<v_k, d> / (|v_k| |d|)``: which modes carry an observed
    conformational change (open -> closed, apo -> holo, snapshot t -> t + dt).  Signed; its square summed over a complete
    set of modes is 1 (:func:`cumulative_overlap`).  ``displacement`` is (N, 3) or (q, N, 3) for an ANM and (N,) or
    (q, N) for a GNM, in the coordinates of the modes: for a mass-weighted model pass ``sqrt(mass)[:, None] * d`` -- this
    function does not do it for you, nor does it superpose the two conformers.  Returns (k,) or (q, k) for the k modes of
    ``mode_subset`` (None: every non-trivial mode; trivial indices raise ValueError, as in :func:`mean_square_fluctuation`).
    A zero displacement gives NaN.  No reference counterpart (ProDy: ``calcOverlap``, Bio3D: ``overlap``); one pass along
    the selected device-resident eigenvectors, only (q, k) numbers cross PCIe.
    """
    d, single = _displacement(enm, displacement)
    if mode_subset is not None:
        mode_subset = _mode_selection(enm, mode_subset, None)   # (the trivial-mode error needs no device)
    modes = enm._modes_device()
    if mode_subset is None:
        mode_subset = _mode_selection(enm, None, modes.order)
    k = np.size(mode_subset)
    out = modes.overlap(mode_subset, d)[0] if k and len(d) else np.empty((len(d), k))
    return out[0] if single else out


def collectivity(enm, mode_subset=None):
    """
    Collectivity of the selected modes (Bruschweiler 1995), ``exp(-sum_a p_a ln p_a) / N`` with ``p_a`` the share of atom
    a in the squared norm of the mode: 1 when every atom moves alike (a rigid translation), 1 / N for a mode on a single
    atom.  (k,) for the k modes of ``mode_subset``, chosen as in :func:`overlap`.  No reference counterpart (ProDy:
    ``calcCollectivity``); same pass as :func:`overlap`.
    """
    _model_kind(enm)
    if mode_subset is not None:
        mode_subset = _mode_selection(enm, mode_subset, None)
    modes = enm._modes_device()
    if mode_subset is None:
        mode_subset = _mode_selection(enm, None, modes.order)
    if not np.size(mode_subset):
        return np.empty(0)
    return modes.overlap(mode_subset, None, collectivity=True)[1]


def cumulative_overlap(overlap):
    """
    ``sqrt(cumsum(overlap**2))`` along the last (mode) axis: the share of a displacement the first k modes describe; over
    a complete orthonormal set it ends at 1.  Pure array arithmetic on a NumPy array or a torch tensor (which stays on
    its device).  No reference counterpart (ProDy: ``calcCumulOverlap``).
    """
    if hasattr(overlap, "cumsum") and not isinstance(overlap, np.ndarray):   # a torch tensor
        return (overlap * overlap).cumsum(-1).sqrt()
    o = np.asarray(overlap, dtype=np.float64)
    return np.sqrt(np.cumsum(o * o, axis=-1))


def distance_fluctuation(enm, mode_subset=None, projected=True, tem=None, tem_factors=K_B):
    """
    Fluctuation of every inter-atom distance over the selected modes, (N, N), symmetric with a zero diagonal:

        ``F[a, c] = <(delta d_ac)^2> = sum_k (n_ac . (v_k[c] - v_k[a]))^2 / lambda_k``,  ``n_ac = (x_c - x_a) / |x_c - x_a|``

    the relative displacement of the two atoms projected on the line between them.  ``k_B T / F`` is the harmonic constant
    of that distance's potential of mean force (:func:`effective_stiffness`): contact-stability and mechanical-resistance
    maps, comparison with distance restraints.  No reference counterpart (ProDy: ``calcDistFlucts``, ``calcMechStiff``;
    Bio3D derives it from the covariance).

    ``mode_subset``, ``tem`` and ``tem_factors`` as in :func:`mean_square_fluctuation`: None takes every non-trivial mode,
    trivial indices raise ValueError.  ``projected=True`` (ANM only; a GNM has no directions and raises ValueError) sums
    the pairs directly on the device-resident eigenvectors (``csrc/dist_fluct.hip``): only non-negative terms, ``F`` and
    ``F.T`` equal bit for bit, the diagonal exactly 0, NaN for two distinct atoms at one position.  The modes enter as
    they are: for a model with masses they are mass-weighted, and the Cartesian figure is what a batch solver returns for
    ``atom_scale=solver.inv_sqrt_mass`` (:meth:`DeviceBatchSolver.distance_fluctuation`).
    ``projected=False`` is ProDy's ``calcDistFlucts``, ``c_aa + c_cc - 2 c_ac`` of the unnormalised :func:`dcc` over the
    same explicit selection, the mean square of the whole relative displacement (for an ANM the sum of the projected
    figure over three orthogonal directions); it works for GNM and ANM and is array arithmetic on the dcc kernel's result.
    """
    kind, _ = _model_kind(enm)
    if projected and kind != "anm":
        raise ValueError("projected distance fluctuations need the directions of an ANM; use projected=False for a GNM")
    if mode_subset is not None:
        mode_subset = _mode_selection(enm, mode_subset, None)   # (the trivial-mode error needs no device)
    modes = enm._modes_device()
    if mode_subset is None:
        mode_subset = _mode_selection(enm, None, modes.order)
    if projected:
        fluct = modes.distfluct(mode_subset, np.asarray(enm._coord, dtype=np.float64))
    else:
        cov = modes.dcc(mode_subset, False)
        diag = np.diag(cov)
        fluct = (diag[:, None] + diag[None, :]) - 2 * cov
    if tem is not None:
        fluct = fluct * (tem * tem_factors)
    return fluct


def effective_stiffness(fluct, tem=None, tem_factors=K_B):
    """
    Harmonic constant of every distance's potential of mean force, ``(tem * tem_factors) / F`` for the fluctuations ``F``
    of :func:`distance_fluctuation` taken without ``tem`` (``1 / F`` when ``tem`` is None, in the units of the force
    constants).  Where ``F`` is 0 -- the diagonal -- the result is exactly 0; NaN stays NaN.  Pure array arithmetic on a
    NumPy array or a torch tensor (which stays on its device).  No reference counterpart (ProDy: ``calcMechStiff``, this
    on the projected fluctuations).
    """
    kt = 1.0 if tem is None else tem * tem_factors
    if hasattr(fluct, "masked_fill") and not isinstance(fluct, np.ndarray):   # a torch tensor
        return (kt / fluct).masked_fill(fluct == 0, 0.0)
    f = np.asarray(fluct, dtype=np.float64)
    out = np.zeros_like(f)
    np.divide(kt, f, out=out, where=f != 0)
    return out


def normal_mode(anm, index, amplitude, frames, movement="sine"):
    """Displacement trajectory (frames, n, 3) for one oscillation of mode ``index`` (nma.py:363-419)."""
    from .anm import ANM

    if not isinstance(anm, ANM):
        raise ValueError("Instance of ANM class expected.")
    _, v = eigen(anm)
    mode = v[index].reshape(-1, 3)
    mode = mode * (amplitude / np.sqrt((mode**2).sum(axis=-1)).max())
    phase = np.linspace(0, 1, frames, endpoint=False)
    if movement == "sine":
        scale = np.sin(phase * 2 * np.pi)
    elif movement == "triangle":
        # triangle wave from -1 (phase 0) over +1 (phase 1/2) back to -1 (nma.py:413)
        scale = 2 * np.abs(2 * (phase - np.floor(phase + 0.5))) - 1
    else:
        raise ValueError(f"Movement '{movement}' is unknown")
    return scale[:, None, None] * mode[None, :, :]


def linear_response(anm, force, mode_subset=None):
    """
    Linear-response displacement covariance . force (nma.py:422-473).  ``force`` is (N, 3) or (3N,) and the result
    (N, 3); q forces at once as (q, N, 3) give (q, N, 3) (extension).

    ``mode_subset=None`` is the reference: the covariance is ``pinv(hessian, rcond=1e-6)`` (anm.py:114-117), every mode
    with ``|lambda| > 1e-6 max|lambda|``.  It is applied in mode space, ``sum_k v_k <v_k, f> / lambda_k`` on the
    device-resident eigenpairs (``csrc/mode_response.hip``): the (3N, 3N) matrix is neither formed nor copied.  A
    covariance that is already on the model -- assigned by the caller or fetched earlier -- is used as it is, like
    :func:`prs` does.  ``mode_subset`` (extension) restricts the sum to the listed modes, as in
    :func:`mean_square_fluctuation`: the response carried by those modes alone; trivial indices raise ValueError.
    For a model with masses the modes enter as they are (the reference's ``covariance @ force`` of the mass-weighted
    Hessian); the Cartesian response is what a batch solver returns for ``atom_scale=solver.inv_sqrt_mass``.
    """
    from .anm import ANM

    if not isinstance(anm, ANM):
        raise ValueError("Instance of ANM class expected.")
    force = np.asarray(force)
    n3 = 3 * len(anm._coord)
    single = force.ndim != 3
    if force.ndim == 3:
        if force.shape[1:] != (n3 // 3, 3):
            raise ValueError(f"Expected forces with shape {('q', n3 // 3, 3)}, got {force.shape}")
        force = force.reshape(force.shape[0], n3)
    elif force.ndim == 2:
        if force.shape != (n3 // 3, 3):
            raise ValueError(f"Expected force with shape {(n3 // 3, 3)}, got {force.shape}")
        force = force.ravel()
    elif force.ndim == 1:
        if len(force) != n3:
            raise ValueError(f"Expected force with length {n3}, got {len(force)}")
    else:
        raise ValueError(f"Expected 1D or 2D array, got {force.ndim} dimensions")
    if mode_subset is not None:
        mode_subset = _mode_selection(anm, mode_subset, None)   # (the trivial-mode error needs no device)
    if mode_subset is None and anm._covariance is not None:
        # a covariance the caller assigned (or already fetched): apply that very matrix
        out = force @ anm._covariance.T if force.ndim == 2 else anm._covariance @ force
    else:
        f = np.ascontiguousarray(force.reshape(-1, n3), dtype=np.float64)
        out = anm._modes_device().response(mode_subset, f, rcond=1e-6) if len(f) else np.empty((0, n3))
    return out.reshape(n3 // 3, 3) if single else out.reshape(len(out), n3 // 3, 3)


def _subset_indices(enm, mode_subset):
    """The selected mode indices as an int64 array (None: every non-trivial mode); host arithmetic only."""
    _, ntriv = _model_kind(enm)
    if mode_subset is None:
        return np.arange(ntriv, len(enm._coord) * enm._dim)
    return np.asarray(_mode_selection(enm, mode_subset, None)).astype(np.int64).reshape(-1)


def mode_displacement(enm, coefficients, mode_subset=None):
    """
    Displacement field ``sum_k c_k v_k`` over the k selected modes: a structure moved along chosen modes, a sample of
    the ensemble (:func:`sample_displacements`), or a displacement put together again from its projections -- with
    ``|d| * overlap(d)`` as coefficients over all modes it is the inverse of :func:`overlap`.  ``coefficients`` is (k,)
    or (q, k), one per mode of ``mode_subset`` in its order (None: every non-trivial mode; trivial indices raise
    ValueError, as in :func:`mean_square_fluctuation`); a wrong length raises ValueError.  Returns (N, 3) or (q, N, 3)
    for an ANM and (N,) or (q, N) for a GNM, in the coordinates of the modes: for a model with masses the modes are
    mass-weighted and ``d / sqrt(mass)[:, None]`` is the Cartesian displacement.  No reference counterpart (ProDy:
    ``deformAtoms``, ``traverseMode``, ``sampleModes``); one pass across the selected device-resident eigenvectors
    (``csrc/mode_response.hip``), only (q, k) numbers go to the device and (q, dim N) come back.
    """
    kind, _ = _model_kind(enm)
    idx = _subset_indices(enm, mode_subset)
    c = np.asarray(coefficients, dtype=np.float64)
    if c.ndim not in (1, 2) or c.shape[-1] != len(idx):
        raise ValueError(f"Expected coefficients of shape ({len(idx)},) or (q, {len(idx)}), one per selected mode, "
                         f"got {c.shape}")
    single = c.ndim == 1
    c = np.ascontiguousarray(c[None] if single else c)
    n = len(enm._coord)
    out = enm._modes_device().combine(idx, c) if len(c) else np.empty((0, n * enm._dim))
    out = out.reshape((len(c), n, 3) if kind == "anm" else (len(c), n))
    return out[0] if single else out


def sample_displacements(enm, n_samples, mode_subset=None, tem=None, tem_factors=K_B, rng=None):
    """
    ``n_samples`` displacement fields drawn from the harmonic ensemble of the selected modes: :func:`mode_displacement`
    of the coefficients ``xi_k sqrt(kT / lambda_k)`` with ``xi`` standard normal, ``kT = tem * tem_factors`` (1 when
    ``tem`` is None).  Their covariance is kT times the covariance matrix restricted to those modes, so the mean square
    displacement per atom tends to :func:`mean_square_fluctuation`.  ``rng``: a seed or ``numpy.random.Generator``
    (``numpy.random.default_rng(rng)``); the numbers are drawn on the host.  ``mode_subset`` as in
    :func:`mode_displacement`.  Returns (n_samples, N, 3) for an ANM, (n_samples, N) for a GNM.
    No reference counterpart (ProDy: ``sampleModes``).
    """
    _model_kind(enm)
    idx = _subset_indices(enm, mode_subset)
    n_samples = int(n_samples)
    if n_samples < 0:
        raise ValueError(f"n_samples must not be negative, got {n_samples}")
    kt = 1.0 if tem is None else tem * tem_factors
    lam = enm._modes_device().values()[idx]
    xi = np.random.default_rng(rng).standard_normal((n_samples, len(idx)))
    return mode_displacement(enm, xi * np.sqrt(kt / lam), idx)


def _pair_operator(enm):
    """The model's :class:`~springcraft_amd.PairOperator`, built once from its coordinates, force field and masses."""
    op = getattr(enm, "_pair_operator", None)
    if op is None:
        from .pair_operator import PairOperator

        op = enm._pair_operator = PairOperator(enm._coord, enm._ff, dim=enm._dim, masses=enm._masses)
    return op


def _selected_modes(enm, mode_subset):
    """Rows (k, dim N) of the selected modes on the host; the selection is :func:`mean_square_fluctuation`'s."""
    _model_kind(enm)
    if mode_subset is not None:
        mode_subset = _mode_selection(enm, mode_subset, None)   # (the trivial-mode error needs no device)
    modes = enm._modes_device()
    if mode_subset is None:
        mode_subset = _mode_selection(enm, None, modes.order)
    _, v = modes.eigen()
    return np.ascontiguousarray(v[np.asarray(mode_subset, dtype=np.int64).reshape(-1)])


def deformation_energy(enm, mode_subset=None):
    """
    Hinsen's per-atom deformation energy of the k selected modes, (k, N):

        ``E_k[a] = 1/2 sum_c gamma_ac (n_ac . (u_k[a] - u_k[c]))^2``  (GNM: without the direction ``n_ac``)

    over the contacts c of atom a, ``u_k`` the mode (divided by ``sqrt(mass)`` for a model with masses): where mode k
    deforms the network rather than moving it rigidly -- hinges and strained regions score high, rigid domains low.  A row
    sums to its eigenvalue.  ``mode_subset`` as in :func:`mean_square_fluctuation` (None: every non-trivial mode; trivial
    indices raise ValueError).  No reference counterpart (Bio3D: ``deformation.nma``).  The sums run on the device from
    the model's own pair list (``csrc/pair_operator.hip``); the operator is built from the model's coordinates, force
    field and masses -- not from a matrix the caller assigned -- and is kept on the model.  Asymmetric force constants
    raise ValueError.
    """
    v = _selected_modes(enm, mode_subset)
    n = len(enm._coord)
    if not len(v):
        return np.empty((0, n))
    return _pair_operator(enm).energy(v).cpu().numpy()


def spring_strain(enm, mode_subset=None):
    """
    What every spring stores in the k selected modes: ``(springs, strain)``, ``springs`` (P, 2) the contacts with
    ``i < j`` and ``strain[k, s] = gamma_s (n_s . (u_k[i] - u_k[j]))^2`` (k, P).  A row sums to its eigenvalue, and
    ``strain[k, s]`` is the first-order change of eigenvalue k per relative change of spring s' constant,
    ``d lambda_k / d ln gamma_s``: which contacts the mode depends on.  Selection, operator and errors as for
    :func:`deformation_energy`.  No reference counterpart.
    """
    v = _selected_modes(enm, mode_subset)
    op = _pair_operator(enm)
    if not len(v):
        return op.springs, np.empty((0, len(op.springs)))
    return op.springs, op.strain(v).cpu().numpy()


def prs(anm, norm=True, mode_subset=None):
    """
    Perturbation-response-scanning matrix from the squared covariance (nma.py:476-524).

    ``mode_subset=None`` is the reference: the covariance is ``pinv(hessian, rcond=1e-6)``, or the matrix the caller
    assigned.  ``mode_subset`` (extension) scans the covariance restricted to the listed modes, ``sum_k v_k v_k^T /
    lambda_k``, as in :func:`mean_square_fluctuation`: trivial indices raise ValueError, a mode listed twice counts twice.
    That matrix is never formed: its 3 x 3 blocks are summed and squared in registers on the device-resident eigenpairs
    (``csrc/mode_prs.hip``, the kernel of the batch solvers' ``prs``).  It cannot be combined with an assigned covariance,
    which has no modes: ValueError.
    """
    from .anm import ANM

    if not isinstance(anm, ANM):
        raise ValueError("Instance of ANM class expected.")
    if mode_subset is not None:
        mode_subset = _mode_selection(anm, mode_subset, None)   # (the trivial-mode error needs no device)
        if anm._covariance is not None:
            raise ValueError("mode_subset cannot be combined with a covariance that is already on the model: "
                             "that matrix has no modes to select from")
        return anm._modes_device().prs_subset(mode_subset, norm)
    if anm._covariance is not None:
        # a covariance the caller assigned (or already fetched): reduce that very matrix
        c2 = anm._covariance**2
        n = c2.shape[0] // 3
        mat = c2.reshape(n, 3, n, 3).sum(axis=(1, 3))
        if norm:
            mat = mat / np.diag(mat)[:, None]
        return mat
    # covariance = pinv(hessian, rcond=1e-6) (anm.py:114-117) formed and reduced on the device
    return anm._modes_device().prs(1e-6, norm)


def generalized_correlation(anm, mode_subset=None, information=False):
    """
    (n, n) generalized correlation coefficients of Lange & Grubmueller (2006) from the linear mutual information of every
    atom pair: how much atom c knows about atom a's motion, whatever the directions.  :func:`dcc` keeps the trace of the
    3 x 3 covariance block ``C_ac`` and is 0 for two atoms that move in lockstep along perpendicular lines; here

        ``C_ac = sum_k v_k[a] v_k[c]^T / lambda_k``,  ``C_aa = L_a L_a^T``,  ``M = L_a^-1 C_ac L_c^-T``
        ``delta = det(I - M M^T)`` clamped to [0, 1],  ``I = -1/2 ln(delta)`` (nats),  ``r = sqrt(1 - delta^(1/3))``

    which is ``1/2 [ln det C_aa + ln det C_cc - ln det C_(ac)]`` on the 6 x 6 block and ``r = sqrt(1 - exp(-2 I / 3))``.
    ``information=True`` returns I instead of r.  No reference counterpart (Bio3D: ``lmi`` / ``dccm(method="lmi")``,
    correlationplus).  The selection is :func:`dcc`'s: ``mode_subset=None`` takes the covariance rule, every mode with
    ``|lambda| > 1e-6 max|lambda|``; trivial indices raise ValueError.

    r and I do not change under any invertible linear map per atom, so there is no ``tem`` / ``tem_factors`` and a model
    with masses gives the Cartesian result as it is.  ``r[a, a]`` is 1.0 and ``I[a, a]`` +inf by definition; an atom whose
    own block cannot be whitened (a Cholesky pivot not finite or <= 2^-40 times the block's diagonal entry: fewer than
    three modes, an atom at rest in the selection) has NaN in its row and column; exactly three modes give r = 1 up to
    rounding.  ANM only -- for a GNM r is ``abs(dcc(norm=True))``.  Computed on the device-resident eigenpairs by the
    batch solvers' kernel (``csrc/mode_lmi.hip``) with a batch of one: no covariance is formed.
    """
    from .anm import ANM

    if not isinstance(anm, ANM):
        raise ValueError("Instance of ANM class expected: for a GNM the generalized correlation is abs(dcc(norm=True))")
    if mode_subset is not None:
        mode_subset = _mode_selection(anm, mode_subset, None)   # (the trivial-mode error needs no device)
    return anm._modes_device().lmi(mode_subset, information)


def correlation_network(enm, kind="dcc", mode_subset=None, contact_cutoff=None, min_correlation=0.0):
    """
    The :class:`~springcraft_amd.network.CorrelationNetwork` of one model's coupling map: ``kind="dcc"`` takes
    ``dcc(enm, mode_subset, norm=True)``, ``kind="lmi"`` ``generalized_correlation(enm, mode_subset)`` (ANM only, its
    ValueError otherwise), and :func:`springcraft_amd.network.correlation_network` turns the map into edge weights
    ``-log|c_ac|``, the shortest path between every pair of atoms and the atoms' path usage on the device.  With
    ``contact_cutoff`` only atoms of the model within that distance are joined.  No reference counterpart (Bio3D: ``cna``).
    The network's arrays are NumPy arrays, like the map.
    """
    from . import network as _net

    _net.check_network_args(min_correlation, contact_cutoff, contact_cutoff is not None)
    if kind not in ("dcc", "lmi"):
        raise ValueError(f"kind must be 'dcc' or 'lmi', got {kind!r}")
    corr = dcc(enm, mode_subset, norm=True) if kind == "dcc" else generalized_correlation(enm, mode_subset)
    coord = None if contact_cutoff is None else np.asarray(enm._coord, dtype=np.float64)
    return _net.correlation_network(corr, coord, contact_cutoff, min_correlation)


def _comparable(enm_a, enm_b):
    """Two models whose modes share their coordinates: the same class and atom count, else ValueError (host only)."""
    _model_kind(enm_a)
    _model_kind(enm_b)
    if type(enm_a) is not type(enm_b):
        raise ValueError(f"Cannot compare the modes of a {type(enm_a).__name__} with those of a {type(enm_b).__name__}")
    if len(enm_a._coord) != len(enm_b._coord):
        raise ValueError(f"Cannot compare the modes of models with {len(enm_a._coord)} and {len(enm_b._coord)} atoms: "
                         "structures of different size have no common coordinates")


def _two_modes(enm_a, enm_b):
    """The device-resident eigenpairs of both models at once (one object when the models are one)."""
    ma = enm_a._modes_device()
    mb = ma if enm_b is enm_a else enm_b._modes_device()
    if not ma._h:
        # (the byte-bounded cache of _model.py released the first model's eigenpairs to keep the second's)
        raise MemoryError("the eigenpairs of both models do not fit the device cache together: raise "
                          "SPRINGCRAFT_MODES_CACHE_BYTES")
    return ma, mb


def _checked_subset(enm, mode_subset):
    """``mode_subset`` as an int64 list with the trivial-mode error of :func:`mean_square_fluctuation`; host only."""
    return np.asarray(_mode_selection(enm, mode_subset, None)).astype(np.int64).reshape(-1)


def rmsip(enm_a, enm_b, n_modes=10, mode_subset=None):
    """
    Root mean square inner product of two models' mode subspaces (Amadei 1999; Bio3D ``rmsip``, ProDy
    ``calcSubspaceOverlap``): ``sqrt(1/k sum_ij <a_i, b_j>^2)`` over the first ``n_modes`` non-trivial modes of each
    (fewer if a model has fewer), or over ``mode_subset`` of both (trivial indices raise ValueError); 1 for equal
    subspaces.  The two models must be of one class and atom count (ValueError).  The modes are compared as they are: for
    models with masses these are the mass-weighted modes (Cartesian modes are not orthonormal; no renormalisation is
    done).  No reference counterpart.  One kernel on the two models' device-resident eigenpairs
    (``csrc/mode_subspace.hip``); one number crosses PCIe.
    """
    _comparable(enm_a, enm_b)
    _, ntriv = _model_kind(enm_a)
    if mode_subset is None:
        n_modes = int(n_modes)
        if n_modes < 0:
            raise ValueError(f"n_modes must not be negative, got {n_modes}")
        idx = np.arange(ntriv, min(ntriv + n_modes, len(enm_a._coord) * enm_a._dim))
    else:
        idx = _checked_subset(enm_a, mode_subset)
    ma, mb = _two_modes(enm_a, enm_b)
    return ma.subspace(mb, idx, idx, 0)[0]


def covariance_overlap(enm_a, enm_b, mode_subset=None):
    """
    Covariance overlap of two models (Hess 2002; Bio3D ``covsoverlap``, ProDy ``calcCovOverlap``): ``1 - sqrt(max(0, tr A +
    tr B - 2 tr(sqrt(A) sqrt(B))) / (tr A + tr B))`` for the covariances ``A = sum_i a_i a_i^T / lambda_i`` over the selected
    modes; 1 for equal covariances.  ``mode_subset=None`` takes, per model, the covariance rule of :func:`dcc`: every mode
    with ``|lambda| > 1e-6 max|lambda|``.  Models, masses and kernel as in :func:`rmsip`.
    """
    _comparable(enm_a, enm_b)
    idx = None if mode_subset is None else _checked_subset(enm_a, mode_subset)
    ma, mb = _two_modes(enm_a, enm_b)
    return ma.subspace(mb, idx, idx, 1, rcond=1e-6)[0]


def mode_overlap_matrix(enm_a, enm_b, mode_subset_a, mode_subset_b=None):
    """
    (k_a, k_b) table of the overlaps ``<a_i, b_j>`` of the listed modes of two models, the table one matches modes with
    (ProDy ``calcOverlap(modesA, modesB)``); ``mode_subset_b=None`` takes ``mode_subset_a`` for both.  Signed; the rows of
    a model's modes are unit vectors.  Models and kernel as in :func:`rmsip`; only (k_a, k_b) numbers cross PCIe.
    """
    _comparable(enm_a, enm_b)
    ia = _checked_subset(enm_a, mode_subset_a)
    ib = ia if mode_subset_b is None else _checked_subset(enm_b, mode_subset_b)
    if not len(ia) or not len(ib):
        return np.empty((len(ia), len(ib)))
    ma, mb = _two_modes(enm_a, enm_b)
    return ma.subspace(mb, ia, ib, 0, gram=True)[1]


def effector_sensor(prs_matrix):
    """Row / column means of the off-diagonal PRS entries (nma.py:527-569)."""
    m = np.array(prs_matrix, dtype=float)
    n = len(m)
    off = m - np.diag(np.diag(m))
    return off.sum(axis=1) / (n - 1), off.sum(axis=0) / (n - 1)
