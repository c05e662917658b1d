"""
The exact lowest modes of a network too large for its dense matrix: Chebyshev-filtered subspace iteration (Zhou & Saad
2006; Zhou, Saad, Tiago & Chelikowsky 2006) on the pair-list operator, in memory of order (dim N, k).  The reference has
no counterpart.

A block of ``nb = k + guard`` columns is filtered by a Chebyshev polynomial in ``H`` that damps the unwanted interval
``[a, b]`` and is normalised at ``a0``, orthonormalised, and rotated to Ritz vectors, until the residuals of the k lowest
pairs are at most ``tol * b``.  With ``e = (b - a) / 2``, ``c = (b + a) / 2``, ``sigma_1 = e / (a0 - c)`` the filter is
the scaled three-term recurrence ::

    Y_1      = (sigma_1 / e) (H X - c X)
    sigma_j+1 = 1 / (2 / sigma_1 - sigma_j)
    Y_j+1    = (2 sigma_j+1 / e) (H Y_j - c Y_j) - sigma_j sigma_j+1 Y_j-1

and every step is ONE call ``Z <- alpha H X + beta X + gamma_c Z`` of the panel kernel (``csrc/pair_panel.hip``,
:meth:`PairOperator.panel_step`) that ping-pongs two buffers, ``Z`` holding ``Y_j-1``.  ``b`` comes from
:func:`spectral_bound`, a guaranteed bound that costs nothing, ``a0`` and ``a`` are the lowest and the highest Ritz value
of the block.

:func:`chebyshev_subspace_iteration` is written against two callables -- the panel step and a small symmetric
eigensolver -- and torch tensors on any device; the tall-skinny products go through ``torch.matmul``.
:func:`spectral_bound` and :func:`filter_coefficients` are host code and need no GPU.  Users reach the solver through
:meth:`PairOperator.lowest_modes` and :meth:`RTB.refine`.
"""

import math

import numpy as np

__all__ = ["spectral_bound", "filter_coefficients", "default_guard", "chebyshev_subspace_iteration", "checked_block",
           "start_block"]


def spectral_bound(pairs, gamma, n_atoms, inv_sqrt_mass=None):
    """
    ``b = 2 max_i t_i^2 sum_{p = (i, .)} |gamma_p|``, an upper bound of the largest eigenvalue (in magnitude) of the
    matrix ``T H T`` of the directed pair list ``pairs`` (k, 2), ``gamma`` (k,), ``t = inv_sqrt_mass`` (n_atoms,) or 1.

    ``x^T T H T x = sum_springs gamma (n . (u_i - u_j))^2`` with ``u = T x``; ``(n . (u_i - u_j))^2 <= 2 (|u_i|^2 +
    |u_j|^2)``, and the sum over springs of ``|gamma| (|u_i|^2 + |u_j|^2)`` counts every atom's directed pairs once, so
    ``|x^T T H T x| <= 2 sum_i |u_i|^2 sum_{p = (i, .)} |gamma_p| <= b |x|^2``.  Host NumPy, deterministic, no Lanczos run.
    """
    n_atoms = int(n_atoms)
    p = np.asarray(pairs)
    g = np.abs(np.asarray(gamma, dtype=np.float64))
    if p.ndim != 2 or p.shape[1] != 2 or g.shape != (len(p),):
        raise ValueError(f"Expected pairs (k,2) and gamma (k,), got {p.shape} and {g.shape}")
    row = np.bincount(p[:, 0].astype(np.int64), weights=g, minlength=n_atoms) if len(p) else np.zeros(n_atoms)
    if inv_sqrt_mass is not None:
        t = np.asarray(inv_sqrt_mass, dtype=np.float64)
        if t.shape != (n_atoms,):
            raise IndexError(f"{t.shape} mass factors for {n_atoms} atoms given")
        row = row * t * t
    return 2.0 * float(row.max()) if n_atoms else 0.0


def filter_coefficients(a0, a, b, degree):
    """
    The ``degree`` triples ``(alpha, beta, gamma_c)`` of the panel steps ``Y_j <- alpha H Y_j-1 + beta Y_j-1 + gamma_c
    Y_j-2`` (``Y_0 = X``; the first has ``gamma_c = 0``) whose last result is ``T_d((H - c) / e) / T_d((a0 - c) / e) X``:
    the Chebyshev polynomial that stays within ``1 / |T_d((a0 - c) / e)|`` on ``[a, b]`` and is 1 at ``a0 < a``.
    """
    a0, a, b, degree = float(a0), float(a), float(b), int(degree)
    if degree < 1:
        raise ValueError(f"the filter degree must be at least 1, got {degree}")
    if not a0 < a < b:
        raise ValueError(f"the filter needs a0 < a < b, got {a0}, {a}, {b}")
    e, c = (b - a) / 2.0, (b + a) / 2.0
    sigma1 = e / (a0 - c)
    steps = [(sigma1 / e, -c * sigma1 / e, 0.0)]
    sigma = sigma1
    for _ in range(degree - 1):
        nxt = 1.0 / (2.0 / sigma1 - sigma)
        steps.append((2.0 * nxt / e, -2.0 * nxt * c / e, -sigma * nxt))
        sigma = nxt
    return steps


def default_guard(k):
    """
    Guard columns beyond the k wanted ones: ``max(8, ceil(k / 4))``.  The filter separates the wanted end of the block
    from its highest Ritz value, so the convergence rate of mode k - 1 is set by the gap ``lambda_nb - lambda_k-1``: eight
    columns keep it open for small k, a quarter of k follows the density of a growing spectrum.
    """
    return max(8, -(-int(k) // 4))


def checked_block(k, guard, m):
    """(k, guard, nb) of a solve of order m, or ValueError."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    guard = default_guard(k) if guard is None else int(guard)
    if guard < 0:
        raise ValueError(f"guard must not be negative, got {guard}")
    if k + guard > m:
        raise ValueError(f"k + guard = {k + guard} columns exceed the order {m} of the matrix: take the dense solver")
    return k, guard, k + guard


def start_block(start, m, nb, seed):
    """
    The (m, nb) float64 starting panel on the host: the rows of ``start`` (k', m), k' >= 1, as its first columns --
    truncated to nb, or padded with standard-normal columns of ``RandomState(seed)`` -- or all random for None.
    """
    rng = np.random.RandomState(seed)
    if start is None:
        return rng.standard_normal((m, nb))
    s = np.asarray(start, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] != m:
        raise ValueError(f"Expected start rows of shape (k', {m}) with k' >= 1, got {s.shape}")
    x = np.empty((m, nb))
    have = min(len(s), nb)
    x[:, :have] = s[:have].T
    if have < nb:
        # the rows' own scale, so that the first Gram matrix is not graded by the padding
        x[:, have:] = rng.standard_normal((m, nb - have)) * (np.linalg.norm(s[:have]) / math.sqrt(have * m) or 1.0)
    return x


def _orthonormalise(x, small_eigh):
    """
    ``X (X^T X)^(-1/2)`` up to a rotation, through the eigendecomposition of the (nb, nb) Gram matrix.  One pass leaves
    ``|X^T X - I|`` of the order ``eps cond(X)^2``, 7e-11 after a filter of degree 40: the callers run two.
    """
    import torch

    g = x.T @ x
    s, u = small_eigh((g + g.T) * 0.5)
    # (a direction the filter annihilated: kept finite, the second pass and the Ritz step sort it to the block's top)
    s = torch.maximum(s, s.abs().max() * 1e-30)
    return x @ (u / torch.sqrt(s)[None, :])


def chebyshev_subspace_iteration(panel_step, small_eigh, x0, k, b, tol=1e-8, degree=20, max_iter=100):
    """
    The k lowest eigenpairs of a symmetric operator with spectrum inside ``[-b, b]`` from the starting panel ``x0`` (m, nb),
    nb >= k, a contiguous float64 torch tensor on the device the callables work on.

    ``panel_step(X, Z, alpha, beta, gamma_c)`` performs ``Z <- alpha H X + beta X + gamma_c Z`` on contiguous (m, nb)
    tensors (``Z`` is not ``X``; with ``gamma_c = 0`` its content is not read).  ``small_eigh(A)`` returns ``(w, U)`` of a
    symmetric (nb, nb) tensor, ascending, eigenvectors as columns, and may destroy ``A``.

    Returns ``(w (k,), x (m, k), info)``: Ritz values ascending, orthonormal Ritz vectors as columns, and ``info`` with
    ``iterations`` (filter passes), ``panel_steps`` (calls of ``panel_step``), ``residuals`` (k,) host array ``|H x - w x|``,
    ``b``, ``tol`` and ``converged`` (all k residuals ``<= tol * b``).  After ``max_iter`` filter passes without convergence
    the current pairs are returned with ``converged = False``; nothing is raised.
    """
    import torch

    nb = x0.shape[1]
    if not 1 <= k <= nb:
        raise ValueError(f"k = {k} outside 1..{nb}, the columns of the starting panel")
    b = float(b)
    x, steps, iterations = x0, 0, 0
    while True:
        x = _orthonormalise(_orthonormalise(x, small_eigh), small_eigh)
        hx = torch.empty_like(x)
        panel_step(x, hx, 1.0, 0.0, 0.0)
        steps += 1
        a = x.T @ hx
        theta, c = small_eigh((a + a.T) * 0.5)
        x, hx = x @ c, hx @ c
        res = torch.linalg.vector_norm(hx - x * theta[None, :], dim=0)
        host = torch.cat([res[:k], theta[:1], theta[-1:]]).cpu().numpy()   # (the one synchronisation of a pass)
        res_k, lowest, highest = host[:k], float(host[k]), float(host[k + 1])
        converged = bool(np.all(res_k <= tol * b))   # (a NaN never converges)
        if converged or iterations >= max_iter:
            break
        upper = highest if highest > lowest else lowest + 1e-3 * b
        if not (np.isfinite(lowest) and lowest < upper < b):
            break   # a non-finite block, or Ritz values at the bound (b = 0: nothing to separate): no filter exists
        y, z = x, hx   # (hx is free now: the two buffers of the recurrence)
        for alpha, beta, gamma_c in filter_coefficients(lowest, upper, b, degree):
            panel_step(y, z, alpha, beta, gamma_c)
            y, z = z, y
        steps += degree
        iterations += 1
        x = y
    info = {"iterations": iterations, "panel_steps": steps, "residuals": res_k.copy(), "b": b, "tol": float(tol),
            "converged": converged}
    return theta[:k], x[:, :k], info
