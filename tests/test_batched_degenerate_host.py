"""
Host test of the member zoo of tests/test_batched_degenerate_gpu.py (tests.util.degenerate_members): every member is what
its name claims, and LAPACK alone meets the gates the GPU tests apply to every member -- with a factor of 100 to spare, so
that a failure on the device is the device's.
"""
import numpy as np
import pytest

from tests.util import degenerate_members

NAMES = ["random", "identity", "zero", "diag", "tridiag", "band40", "band64", "band65", "blockdiag", "rank1", "clustered",
         "nearclustered", "graded", "gluedW", "big", "small", "kirchhoff"]
EXACT = ["identity", "zero", "diag", "rank1", "clustered", "kirchhoff"]


@pytest.fixture(scope="module", params=[322, 1030])
def zoo(request):
    n = request.param
    members, exact = degenerate_members(n, 1)
    return n, members, exact


def half_width(a):
    i, j = np.nonzero(a)
    return int(np.abs(i - j).max()) if len(i) else 0


def test_members_and_their_order(zoo):
    n, members, exact = zoo
    assert [name for name, _ in members] == NAMES
    assert sorted(exact) == sorted(EXACT)
    for name, a in members:
        assert a.shape == (n, n) and a.dtype == np.float64, name
        assert np.array_equal(a, a.T), name
        assert np.isfinite(a).all(), name
    for name in EXACT:
        assert exact[name].shape == (n,) and np.all(np.diff(exact[name]) >= 0), name
    # the same seed gives the same matrices, another seed others
    again = dict(degenerate_members(n, 1)[0])
    other = dict(degenerate_members(n, 2)[0])
    for name, a in members:
        assert np.array_equal(a, again[name]), name
    assert not np.array_equal(dict(members)["random"], other["random"])
    # a subset comes in the fixed order and holds the same matrices
    sub, sub_exact = degenerate_members(n, 1, names=["clustered", "big", "band65"])
    assert [name for name, _ in sub] == ["band65", "clustered", "big"] and list(sub_exact) == ["clustered"]
    for name, a in sub:
        assert np.array_equal(a, again[name]), name


def test_structure_claims(zoo):
    n, members, _ = zoo
    m = dict(members)
    assert np.array_equal(m["identity"], np.eye(n)) and not m["zero"].any()
    assert half_width(m["diag"]) == 0 and np.count_nonzero(np.diag(m["diag"])) == n
    assert half_width(m["tridiag"]) == 1 and np.count_nonzero(np.diag(m["tridiag"], 1)) == n - 1
    for w in (40, 64, 65):
        a = m[f"band{w}"]
        assert half_width(a) == w
        assert np.count_nonzero(np.diag(a, w)) == n - w      # the outermost diagonal is full
    n1 = n // 2 + 5
    b = m["blockdiag"]
    assert n1 % 64 != 0
    assert not b[n1:, :n1].any() and not b[:n1, n1:].any()
    assert np.count_nonzero(b[:n1, :n1]) == n1 * n1 and np.count_nonzero(b[n1:, n1:]) == (n - n1) ** 2
    k = m["kirchhoff"]
    assert np.array_equal(k, np.rint(k))
    lattice_atoms = int(np.count_nonzero(np.diag(k) < 12.5))
    assert 0.85 * n <= lattice_atoms <= n
    assert not k[:lattice_atoms, :lattice_atoms].sum(axis=0).any()                      # a graph Laplacian
    assert half_width(k[lattice_atoms:, lattice_atoms:]) == 0 and not k[lattice_atoms:, :lattice_atoms].any()
    pad = np.diag(k)[lattice_atoms:]
    assert len(np.unique(pad)) == len(pad) and (len(pad) == 0 or pad.min() > 12.0)      # above 4 + 4 + 4
    assert np.array_equal(m["big"], m["random"] * 1e150) and np.array_equal(m["small"], m["random"] * 1e-150)
    g = m["gluedW"]
    assert np.count_nonzero(np.diag(g) == 30.0) == n - 21 * (n // 21)
    off = np.abs(g[np.triu_indices(n, 1)])
    assert np.count_nonzero(off == 1e-10) == n // 21 - 1 and np.count_nonzero(off == 1.0) == 20 * (n // 21)
    assert half_width(g) > 64                                                           # the permutation hides the band


def test_lapack_meets_the_gates_with_a_factor_100_to_spare(zoo):
    """
    Eigenvalues 1e-11 max(lambda_max, tiny), residual 1e-10 max(lambda_max, 1) (`big`, `small`: their own lambda_max),
    orthogonality 1e-11 -- the gates of the GPU module -- each divided by 100, on np.linalg.eigh; the eigenvalues against
    np.linalg.eigvalsh (another LAPACK algorithm) and against the closed form where there is one.
    """
    n, members, exact = zoo
    worst = {"eig": (0.0, ""), "res": (0.0, ""), "orth": (0.0, "")}
    for name, a in members:
        w, v = np.linalg.eigh(a)
        w_ref = np.linalg.eigvalsh(a)
        lam = np.abs(w_ref).max()
        eig = np.abs(w - w_ref).max()
        if name in exact:
            eig = max(eig, np.abs(w - exact[name]).max(), np.abs(w_ref - exact[name]).max())
        assert eig <= 1e-13 * max(lam, 1e-300), (name, eig, lam)
        res = np.abs(a @ v - v * w[None, :]).max()
        res_scale = lam if name in ("big", "small") else max(lam, 1.0)
        assert res <= 1e-12 * res_scale, (name, res, res_scale)
        orth = np.abs(v.T @ v - np.eye(n)).max()
        assert orth <= 1e-13, (name, orth)
        for key, val in (("eig", eig / max(lam, 1e-300)), ("res", res / res_scale), ("orth", orth)):
            if val > worst[key][0]:
                worst[key] = (val, name)
    print(f"n = {n}: LAPACK's worst {worst}")
