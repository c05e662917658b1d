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

The inverse direction, ``(T H T)^+ f`` without the matrix: :func:`conjugate_gradient` on the range of the matrix for q
right-hand sides at once (``csrc/pair_cg.hip``), again a driver against callables.  The null space is known in closed form
(:func:`null_space`), the exact modes of :meth:`PairOperator.lowest_modes` serve as a deflation space.  Users reach it through
:meth:`PairOperator.solve`, ``linear_response``, ``covariance_columns`` and :meth:`RTB.exact_response`.
"""

import math

import numpy as np

__all__ = ["spectral_bound", "filter_coefficients", "default_guard", "chebyshev_subspace_iteration", "checked_block",
           "start_block", "null_space", "checked_solve", "column_dots", "conjugate_gradient", "CG_RUNNING", "CG_CONVERGED",
           "CG_BROKEN_DOWN", "NULL_EIGENVALUE"]


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


# ---- conjugate gradients on the range of the matrix ------------------------------------------------------------------------
CG_RUNNING, CG_CONVERGED, CG_BROKEN_DOWN = 0, 1, 2
NULL_EIGENVALUE = 1e-9   # rows of a deflation space with |w| <= NULL_EIGENVALUE * b count as null vectors


def null_space(coord, dim, inv_sqrt_mass=None):
    """
    An orthonormal basis of the null space of ``T H T`` of a connected network, a host array (dim n, z): for ``dim=3`` the
    six rigid-body fields of ``coord`` (n, 3) divided by ``t = inv_sqrt_mass`` -- :func:`rtb.rtb_projector` with every atom
    in one block, whose columns are exactly these (five for collinear atoms, three for one atom) -- and for ``dim=1`` the
    constant vector divided by ``t`` (``coord`` may then be the atom count).
    """
    if dim not in (1, 3):
        raise ValueError(f"dim must be 1 (GNM) or 3 (ANM), got {dim!r}")
    n = int(coord) if np.ndim(coord) == 0 else len(coord)
    t = None if inv_sqrt_mass is None else np.asarray(inv_sqrt_mass, dtype=np.float64)
    if t is not None and t.shape != (n,):
        raise IndexError(f"{t.shape} mass factors for {n} atoms given")
    if dim == 1:
        z = np.ones((n, 1)) if t is None else (1.0 / t)[:, None]
        return z / np.linalg.norm(z)
    from .rtb import rtb_projector

    proj, _, dof, _ = rtb_projector(coord, np.zeros(n, dtype=np.int64), None if t is None else 1.0 / (t * t))
    return np.ascontiguousarray(proj.reshape(3 * n, 6)[:, : int(dof[0])])


def checked_solve(m, tol, max_iter, check_every, deflate):
    """
    The options of a solve of order m, or ValueError: ``(tol, max_iter, check_every, deflate)`` with ``deflate`` None or
    ``(w (kd,), v (kd, m))`` as they were given (arrays or tensors: only their shapes are read).
    """
    tol = float(tol)
    if not tol > 0.0:
        raise ValueError(f"tol must be positive, got {tol}")
    max_iter, check_every = int(max_iter), int(check_every)
    if max_iter < 0:
        raise ValueError(f"max_iter must not be negative, got {max_iter}")
    if check_every < 1:
        raise ValueError(f"check_every must be at least 1, got {check_every}")
    if deflate is not None:
        if not (isinstance(deflate, (tuple, list)) and len(deflate) == 2):
            raise ValueError("deflate must be a pair (w, v) of eigenvalues (kd,) and eigenvector rows (kd, m)")
        w, v = deflate
        ws, vs = tuple(np.shape(w)), tuple(np.shape(v))
        if len(ws) != 1 or len(vs) != 2 or vs != (ws[0], m):
            raise ValueError(f"deflate must hold eigenvalues (kd,) and eigenvector rows (kd, {m}), got {ws} and {vs}")
        deflate = (w, v)
    return tol, max_iter, check_every, deflate


def _tree_sum(t):
    """The sum over the rows of ``t`` (m, q) by pairwise halving, elementwise operations only; ``t`` is not kept."""
    rows = t.shape[0]
    while rows > 1:
        half = rows // 2
        head = t[:half] + t[half: 2 * half]
        if rows & 1:
            head[0] += t[2 * half]
        t, rows = head, half
    return t[0]


def column_dots(z, f):
    """
    ``z^T f`` (zc, q) of two panels (m, zc) and (m, q) by a pairwise tree of elementwise sums: the order of a column's sums
    depends on m alone, so its bits depend neither on q nor on the other columns (a matrix product promises neither).
    """
    import torch

    if z.shape[1] == 0:
        return f.new_zeros((0, f.shape[1]))
    return torch.stack([_tree_sum(f * z[:, c: c + 1]) for c in range(z.shape[1])])


def _project_out(z, f):
    """``f - z (z^T f)`` in place, column by column in a fixed order (:func:`column_dots`); returns ``f``."""
    coef = column_dots(z, f)
    for c in range(z.shape[1]):
        f -= z[:, c: c + 1] * coef[c][None, :]
    return f


def _iterate(step, read, max_iter, check_every, between=None):
    """Runs ``step`` until no column is running or ``max_iter`` iterations are enqueued; returns the last ``read()``."""
    done = 0
    status, iters, rho = read()
    while done < max_iter and np.any(status == CG_RUNNING):
        count = min(check_every, max_iter - done)
        step(count)
        done += count
        if between is not None:
            between()
        status, iters, rho = read()
    return status, iters, rho


def conjugate_gradient(init, step, f, null, b, tol=1e-8, max_iter=2000, check_every=10, deflate=None, apply=None):
    """
    The minimum-norm solutions ``x = H^+ f`` of a symmetric positive semi-definite operator with the known null space
    ``null`` (m, z), orthonormal columns, for the q columns of ``f`` (m, q): float64 torch tensors on the device the callables
    work on.  ``f`` is overwritten.

    ``X, read = init(R, tol)`` starts a solve from the projected right-hand sides ``R`` (m, q), contiguous: ``X`` (m, q) is
    the tensor the iteration updates, as it updates ``R``, and ``read()`` returns the host arrays ``(status, iters, rho)``,
    each (q,), ``rho = <r, r>``: the one host synchronisation.  ``step(iterations)`` enqueues that many iterations; a
    column stops on its own at ``rho <= (tol |r_0|)^2`` (status 1) or at a breakdown (status 2) and is frozen from then on.

    The driver projects ``f <- f - Z (Z^T f)``, reads the status every ``check_every`` iterations until no column is
    running or ``max_iter`` is reached, and projects ``X`` with ``Z`` at the end.  Without deflation a column's bits depend
    on that column and the operator alone.

    ``deflate = (w (kd,), V (kd, m))``, eigenpairs with the trivial rows first (tensors on the same device), needs
    ``apply(X) -> H X`` on (m, q) panels.  Rows with ``|w| <= 1e-9 b`` count as null vectors; the iteration solves for
    ``f - V^T V f``, re-projects ``R`` against ``V`` at every host check, and the driver adds ``sum_k v_k <v_k, f> / w_k``
    over the other rows (tall-skinny ``torch.matmul``).  Computed eigenpairs are exact to their own residuals only, which
    the closed-form part passes on to the solution: so the driver then forms the true residual ``f_p - H x`` with one
    ``apply`` and, for the columns where it exceeds ``tol |f_p|``, runs a second, undeflated iteration on it down to that
    bound -- a reduction by the small factor the modes' residuals cost, a few iterations, to one relative bound for all
    of these columns, the strictest.  ``max_iter`` bounds each of the two.

    Returns ``(X (m, q), info)``: ``iterations`` (q,), ``residuals`` (q,) = ``sqrt(rho) / |f projected|`` (0 for a zero
    right-hand side), ``status`` (q,), ``converged`` (every status 1), ``b``, ``tol``.  Nothing is raised for a solve that
    runs out of iterations or breaks down.
    """
    import torch

    tol, max_iter, check_every, _ = checked_solve(f.shape[0], tol, max_iter, check_every, None)
    if deflate is not None and apply is None:
        raise ValueError("deflation needs the operator itself: apply(X) -> H X")
    _project_out(null, f)
    fnorm = torch.sqrt(_tree_sum(f * f))
    fh = fnorm.cpu().numpy()
    if deflate is None:
        x, read = init(f, tol)
        status, iters, rho = _iterate(step, read, max_iter, check_every)
        _project_out(null, x)
    else:
        w, v = deflate
        keep = np.abs(w.detach().cpu().numpy()) > NULL_EIGENVALUE * float(b)
        rows = torch.from_numpy(np.nonzero(keep)[0]).to(v.device)
        vt = v.T.contiguous()   # (m, kd), every row: the space R is kept orthogonal to
        fp = f.clone()
        vf = v @ f              # (kd, q)
        f -= vt @ vf

        def reproject():
            f.sub_(vt @ (vt.T @ f))

        x, read = init(f, tol)
        status, iters, rho = _iterate(step, read, max_iter, check_every, reproject)
        x += v[rows].T.contiguous() @ (vf[rows] / w[rows][:, None])
        _project_out(null, x)
        # the true residual, and a second iteration where the modes' own residuals left it above the bound
        r = _project_out(null, fp - apply(x))
        rnorm = torch.sqrt(_tree_sum(r * r))
        rh = rnorm.cpu().numpy()
        rho = rh * rh
        again = (status == CG_CONVERGED) & ~(rh <= tol * fh)
        if np.any(again):
            # one relative bound for the columns that need it, the strictest: |r| tol2 <= tol |f_p| for each of them
            tol2 = max(float(np.min(tol * fh[again] / rh[again])), tol)
            mask = torch.from_numpy(again.astype(np.float64)).to(r.device)
            y, read = init(r * mask[None, :], tol2)   # (the other columns are 0 and stop at once)
            status2, iters2, rho2 = _iterate(step, read, max_iter, check_every)
            x += _project_out(null, y)
            iters = iters + iters2
            status = np.where(again, status2, status)
            rho = np.where(again, rho2, rho)
    with np.errstate(divide="ignore", invalid="ignore"):
        residuals = np.where(fh > 0, np.sqrt(rho) / fh, 0.0)
    info = {"iterations": np.asarray(iters).copy(), "residuals": residuals, "status": np.asarray(status).copy(),
            "converged": bool(np.all(status == CG_CONVERGED)), "b": float(b), "tol": tol}
    return x, info
