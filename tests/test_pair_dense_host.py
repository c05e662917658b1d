"""
Host tests (no GPU) of the networks of tests/test_pair_dense_gpu.py, in which an atom has 63 .. 130 pairs, and of the
iteration caps that file uses.  The walk over an atom's pairs (csrc/pair_walk.h, and ``k_pairs_apply``) takes them 64 at a
time; the networks are the smallest that reach a full chunk, a later chunk, and a skipped row in either.

Dense networks: the first N atoms of a jittered lattice (tests/test_iterative_host.py) under ``HinsenForceField()``, which has
no cutoff, so the list holds every ordered pair, sorted by first then second atom, N - 1 per atom:

    D64   lattice(4, 5, 6, 3)[:64]    63 pairs per atom   one chunk, one short of full
    D65   lattice(4, 5, 6, 3)[:65]    64                  one full chunk
    D66   lattice(4, 5, 6, 3)[:66]    65                  64 + 1
    D129  lattice(6, 6, 8, 4)[:129]   128                 two full chunks
    D131  lattice(6, 6, 8, 4)[:131]   130                 64 + 64 + 2

The list is written down here in NumPy (the package's own scan needs the device; the GPU file asserts that the package
lists exactly these rows); the constants are the package's ``HinsenForceField.force_constant`` on NumPy's squared
distances.  They span more than two decades and both branches of the formula occur, which :func:`test_hinsen_constants`
checks: a pair added at the wrong place is then far outside the gates.

MIX: D66 without the springs (0, 1), (2, 3), (2, 4), both directions: atoms 0 .. 7 have 64, 64, 63, 64, 64, 65, 65, 65 pairs,
so the four wavefronts of the workgroups 0 and 1 make different numbers of trips.

Unchecked lists, for the C entries only (D66's rows and ``row_start`` with some atoms overwritten; the host checks of
``PairOperator.from_pairs`` refuse them).  U1: in atom 5's range the second atom of row 3 is -1 and of row 64 is N, the first
atom of row 10 is 6; in atom 6's range the second atom of row 0 is -1 -- skipped rows inside a full chunk, a one-pair
second chunk that becomes empty, and a chunk's first row.  U2: every row of atom 7 has the second atom -1.  The reference
of either is the restatement of the list without those rows (:func:`unchecked`).

Iteration caps.  The NumPy prototypes of the two drivers (the stand-ins of tests/test_iterative_host.py and
tests/test_solve_host.py, the dense matrix as operator) need, with ``tol = 1e-10``:

    conjugate gradients, seven right-hand sides     D131 plain 148, D131 mass-weighted 184, D66 as a GNM 38 iterations
    lowest_modes(12), degree 20, seed 0             D131 plain 11, D131 mass-weighted 18 passes

The caps ``SOLVE_MAX_ITER = 600`` and ``MODES_MAX_ITER = 60`` are at least three times these, the margin of the files named
above; :func:`test_prototypes_need_a_third_of_the_caps` holds them to it.
"""
import numpy as np
import pytest

from springcraft_amd import HinsenForceField, iterative
from springcraft_amd.pair_operator import check_symmetric, pair_row_start
from tests.test_iterative_host import lattice, masses_of, np_callables, np_matrix
from tests.test_solve_host import check_solution, host_solve, right_hand_sides

DENSE = {"D64": ((4, 5, 6, 3), 64), "D65": ((4, 5, 6, 3), 65), "D66": ((4, 5, 6, 3), 66),
         "D129": ((6, 6, 8, 4), 129), "D131": ((6, 6, 8, 4), 131)}
REMOVED = ((0, 1), (2, 3), (2, 4))       # MIX: the springs taken out of D66
MIX_COUNTS = [64, 64, 63, 64, 64, 65, 65, 65]
TOL, DEGREE, K_MODES = 1e-10, 20, 12
SOLVE_MAX_ITER, MODES_MAX_ITER = 600, 60
END_TO_END = [("D131", False, 3), ("D131", True, 3), ("D66", False, 1)]
END_IDS = ["D131-plain", "D131-mass", "D66-gnm"]


def coord_of(name):
    dims, n = DENSE["D66" if name in ("MIX", "U1", "U2") else name]
    return lattice(*dims)[:n]


def dense_network(name):
    """(coord, pairs, gamma) of a dense network or of MIX: every ordered pair in list order, Hinsen's constants."""
    coord = coord_of(name)
    n = len(coord)
    i, j = np.divmod(np.arange(n * n, dtype=np.int64), n)
    pairs = np.stack([i, j], axis=1)[i != j]
    if name == "MIX":
        gone = np.zeros(len(pairs), dtype=bool)
        for a, b in REMOVED:
            gone |= ((pairs[:, 0] == a) & (pairs[:, 1] == b)) | ((pairs[:, 0] == b) & (pairs[:, 1] == a))
        pairs = pairs[~gone]
    d = coord[pairs[:, 1]] - coord[pairs[:, 0]]
    gamma = np.asarray(HinsenForceField().force_constant(pairs[:, 0], pairs[:, 1], (d * d).sum(axis=1)), dtype=np.float64)
    return coord, np.ascontiguousarray(pairs), gamma


def unchecked(name):
    """
    ``(coord, pairs, gamma, row_start, keep)`` of U1 / U2: D66's list with the overwritten atoms, D66's own ``row_start``, and
    the mask of the rows the kernels must still add (``pairs[keep], gamma[keep]`` is the cleaned list of the reference).
    """
    coord, pairs, gamma = dense_network("D66")
    n = len(coord)
    start = pair_row_start(pairs, n)
    pairs = pairs.copy()
    if name == "U1":
        pairs[start[5] + 3, 1] = -1
        pairs[start[5] + 64, 1] = n
        pairs[start[5] + 10, 0] = 6
        pairs[start[6] + 0, 1] = -1
    elif name == "U2":
        pairs[start[7]: start[8], 1] = -1
    else:
        raise KeyError(name)
    owner = np.repeat(np.arange(n), np.diff(start))
    keep = (pairs[:, 0] == owner) & (pairs[:, 1] >= 0) & (pairs[:, 1] < n)
    return coord, pairs, gamma, start, keep


@pytest.mark.parametrize("name", list(DENSE))
def test_every_atom_of_a_dense_network_has_n_minus_one_pairs(name):
    coord, pairs, gamma = dense_network(name)
    n = DENSE[name][1]
    assert len(coord) == n and len(pairs) == n * (n - 1) == len(gamma)
    assert np.array_equal(np.bincount(pairs[:, 0], minlength=n), np.full(n, n - 1))
    key = pairs[:, 0] * n + pairs[:, 1]
    assert np.all(np.diff(key) > 0)       # sorted by first then second atom, no row twice
    check_symmetric(pairs, gamma, n)
    assert np.array_equal(np.diff(pair_row_start(pairs, n)), np.full(n, n - 1))
    chunks = -(-(n - 1) // 64)
    assert (n - 1, chunks) == {"D64": (63, 1), "D65": (64, 1), "D66": (65, 2), "D129": (128, 2), "D131": (130, 3)}[name]


@pytest.mark.parametrize("name", list(DENSE))
def test_hinsen_constants(name):
    """Both branches of the formula occur and the constants span more than two decades."""
    coord, pairs, gamma = dense_network(name)
    d = np.linalg.norm(coord[pairs[:, 1]] - coord[pairs[:, 0]], axis=1)
    print(f"{name}: distances {d.min():.3f} .. {d.max():.3f} A, {np.count_nonzero(d < 4.0)} rows below 4 A; gamma "
          f"{gamma.min():.4g} .. {gamma.max():.4g}")
    assert d.min() > 2.9 and np.count_nonzero(d < 4.0) >= 20 and np.count_nonzero(d >= 4.0) >= 20
    assert np.all(gamma > 0) and gamma.max() > 100.0 * gamma.min()
    near = d < 4.0
    assert np.allclose(gamma[near], 860.0 * d[near] - 2390.0, rtol=1e-12, atol=0)
    assert np.allclose(gamma[~near], 1.28e6 / d[~near] ** 6, rtol=1e-12, atol=0)


def test_mix_gives_the_wavefronts_of_a_workgroup_different_trip_counts():
    coord, pairs, gamma = dense_network("MIX")
    n = len(coord)
    counts = np.bincount(pairs[:, 0], minlength=n)
    assert n == 66 and len(pairs) == 66 * 65 - 2 * len(REMOVED)
    assert list(counts[:8]) == MIX_COUNTS and np.all(counts[8:] == 65)
    check_symmetric(pairs, gamma, n)       # (raises otherwise)
    full, mixed = dense_network("D66")[1:], set(map(tuple, pairs))
    assert all(tuple(p) in mixed or tuple(sorted(p)) in REMOVED for p in full[0])
    # the constants of the remaining rows are D66's
    rows = np.array([tuple(p) in mixed for p in full[0]])
    assert np.array_equal(gamma, full[1][rows])
    # still one connected network: six zero modes
    lam = np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, 3))
    assert np.all(np.abs(lam[:6]) <= 1e-12 * lam[-1]) and lam[6] > 1e-6 * lam[-1]


def test_unchecked_lists_hold_the_stated_rows_and_the_host_refuses_them():
    n = 66
    _, d66, g66 = dense_network("D66")
    coord, pairs, gamma, start, keep = unchecked("U1")
    assert np.array_equal(start, pair_row_start(d66, n)) and np.array_equal(gamma, g66)
    changed = np.nonzero(np.any(pairs != d66, axis=1))[0]
    assert list(changed) == [5 * 65 + 3, 5 * 65 + 10, 5 * 65 + 64, 6 * 65]
    assert [tuple(p) for p in pairs[changed]] == [(5, -1), (6, 11), (5, n), (6, -1)]
    assert list(np.nonzero(~keep)[0]) == list(changed)
    counts = np.bincount(pairs[keep][:, 0], minlength=n)
    assert counts[5] == 62 and counts[6] == 64 and np.all(np.delete(counts, [5, 6]) == 65)
    # atom 5: the first chunk is full and holds two skipped rows, the second has one row, which is skipped
    assert start[6] - start[5] == 65 and not keep[start[5] + 64] and np.count_nonzero(~keep[start[5]: start[5] + 64]) == 2
    for check in (lambda: check_symmetric(pairs, gamma, n), lambda: pair_row_start(pairs, n)):
        with pytest.raises(ValueError, match="outside"):
            check()
    in_range = pairs.copy()       # the row with the wrong first atom alone is refused as well
    in_range[in_range[:, 1] < 0, 1] = 0
    in_range[in_range[:, 1] >= n, 1] = 0
    with pytest.raises(ValueError):
        check_symmetric(in_range, gamma, n)

    coord, pairs, gamma, start, keep = unchecked("U2")
    assert np.array_equal(np.nonzero(~keep)[0], np.arange(7 * 65, 8 * 65)) and np.all(pairs[~keep, 1] == -1)
    assert np.all(pairs[~keep, 0] == 7) and np.array_equal(pairs[keep], d66[keep])
    assert np.bincount(pairs[keep][:, 0], minlength=n)[7] == 0
    with pytest.raises(ValueError, match="outside"):
        check_symmetric(pairs, gamma, n)


def host_case(name, masses, dim):
    coord, pairs, gamma = dense_network(name)
    n = len(coord)
    scale = 1.0 / np.sqrt(masses_of(n)) if masses else None
    h = np_matrix(coord, pairs, gamma, dim, scale)
    return coord, h, iterative.spectral_bound(pairs, gamma, n, scale), iterative.null_space(coord, dim, scale)


@pytest.mark.parametrize("key", END_TO_END, ids=END_IDS)
def test_prototypes_need_a_third_of_the_caps(key):
    import torch

    name, masses, dim = key
    coord, h, b, z = host_case(name, masses, dim)
    lam = np.linalg.eigvalsh(h)
    assert np.all(np.abs(lam[: z.shape[1]]) <= 1e-12 * lam[-1]) and lam[z.shape[1]] > 1e-6 * lam[-1] and b >= lam[-1]
    f = right_hand_sides(len(coord), dim)
    x, info = host_solve(h, z, b, f, tol=TOL, max_iter=SOLVE_MAX_ITER)
    check_solution(x, info, h, z, b, f, label=f"{name} dim {dim}, NumPy prototype")
    print(f"conjugate gradients: {info['iterations'].max()} iterations, cap {SOLVE_MAX_ITER}")
    assert 3 * info["iterations"].max() <= SOLVE_MAX_ITER
    if dim == 1:
        return
    k, guard, nb = iterative.checked_block(K_MODES, None, len(h))
    panel_step, small_eigh, _ = np_callables(h)
    x0 = torch.from_numpy(iterative.start_block(None, len(h), nb, 0))
    w, v, modes = iterative.chebyshev_subspace_iteration(panel_step, small_eigh, x0, k, b, tol=TOL, degree=DEGREE,
                                                         max_iter=MODES_MAX_ITER)
    print(f"lowest modes: {modes['iterations']} passes, cap {MODES_MAX_ITER}; block {nb} columns, gap "
          f"(lambda[{nb}] - lambda[{k - 1}]) / b = {(lam[nb] - lam[k - 1]) / b:.4f}")
    assert modes["converged"] and 3 * modes["iterations"] <= MODES_MAX_ITER
    assert np.all(np.abs(w.numpy() - lam[:k]) <= TOL * b + 1e-12 * b)
