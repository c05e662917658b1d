"""
The stage ratios of tests/stage_ratios.py applied to LAPACK's own factors, on every input tests/test_stage_ratios_gpu.py
uses: scipy.linalg.hessenberg (dgehrd + dorghr: on a symmetric matrix a tridiagonalisation with its Q) for the reduction,
np.linalg.eigh of the dense T for the tridiagonal solver, np.linalg.eigh(a) for the whole decomposition.  LAPACK must stay
below a tenth of the gate everywhere -- the gate then stands two orders of magnitude above the reference -- and planted
perturbations of 1e-13 / 1e-12 must fail it: the ratios see what the suite's max-abs gates (1e-10, 1e-11) cannot.
(scipy.linalg.eigh_tridiagonal is no reference here: it is MRRR, which reaches orth = 46 on a random T at n = 256.)
"""
import numpy as np
import pytest
import scipy.linalg

from tests import stage_ratios as sr

DENSE_ORDERS = [256, 322, 1030, 2050]     # the batches of one of the GPU tests (2050: the resident kernel's register form)
MIXED_ORDERS = [130, 322]
TRIDIAGONAL_ORDERS = [2, 32, 33, 322, 1000]


def lapack_reduction(a):
    h, q = scipy.linalg.hessenberg(a, calc_q=True)
    return q, sr.tridiagonal(np.diag(h).copy(), np.diag(h, -1).copy())


_factors = {}


def lapack_factors(label, a):
    """(Q, T, w, V) of one input, computed once for the NumPy ratios and their torch twins."""
    key = (label, hash(a.tobytes()))      # (the mixed batch has a member called random too)
    if key not in _factors:
        _factors[key] = lapack_reduction(a) + tuple(np.linalg.eigh(a))
    return _factors[key]


def check_dense(label, a):
    """(reduction recon, orth; eigh recon, orth) of one matrix, all at most LAPACK_GATE."""
    q, t, w, v = lapack_factors(label, a)
    figures = (sr.recon(a, q, t), sr.orth(q), sr.recon(a, v, np.diag(w)), sr.orth(v))
    print(f"[{label}] dgehrd recon {figures[0]:.3f} orth {figures[1]:.3f}   eigh recon {figures[2]:.3f} orth {figures[3]:.3f}")
    assert max(figures) <= sr.LAPACK_GATE, (label, figures)
    return figures


@pytest.mark.parametrize("n", DENSE_ORDERS)
def test_lapack_on_random_matrices(n):
    check_dense(f"random n={n}", sr.random_sym(n))


@pytest.mark.parametrize("n", MIXED_ORDERS)
def test_lapack_on_the_mixed_batch(n):
    names, mats = sr.mixed_batch(n)
    for name, a in zip(names, mats):
        check_dense(f"{name} n={n}", a)


def check_dense_t(label, a):
    """The same four figures by recon_t / orth_t on CPU tensors: the same gate, and the NumPy figures to rounding."""
    import torch

    q, t, w, v = lapack_factors(label, a)
    ta, tq, tt, tv = (torch.tensor(x) for x in (a, q, t, v))
    figures = (sr.recon_t(ta, tq, tt), sr.orth_t(tq), sr.recon_t(ta, tv, torch.diag(torch.from_numpy(w))), sr.orth_t(tv))
    ref = (sr.recon(a, q, t), sr.orth(q), sr.recon(a, v, np.diag(w)), sr.orth(v))
    print(f"[{label}] torch: dgehrd recon {figures[0]:.3f} orth {figures[1]:.3f}   eigh recon {figures[2]:.3f} "
          f"orth {figures[3]:.3f}   (NumPy {ref[0]:.3f} {ref[1]:.3f} {ref[2]:.3f} {ref[3]:.3f})")
    assert max(figures) <= sr.LAPACK_GATE, (label, figures)
    # the two evaluate one formula with other summation orders: they differ by the rounding of the products, about
    # sqrt(n) ulp per entry, i.e. n^-1/2 <= 0.09 of a unit at these orders (n >= 130) -- further apart is another formula
    assert all(abs(f - r) <= 0.1 for f, r in zip(figures, ref)), (label, figures, ref)


@pytest.mark.parametrize("n", DENSE_ORDERS)
def test_torch_ratios_on_random_matrices(n):
    check_dense_t(f"random n={n}", sr.random_sym(n))


@pytest.mark.parametrize("n", MIXED_ORDERS)
def test_torch_ratios_on_the_mixed_batch(n):
    names, mats = sr.mixed_batch(n)
    for name, a in zip(names, mats):
        check_dense_t(f"{name} n={n}", a)


def test_torch_ratios_see_planted_perturbations():
    import torch

    n = 256
    a = sr.random_sym(n)
    q, t, _, _ = lapack_factors(f"random n={n}", a)
    bad_q = torch.from_numpy(q + 1e-13 * np.random.RandomState(5).randn(n, n))
    assert sr.orth_t(bad_q) > sr.GATE
    bad_t = t.copy()
    bad_t[n // 2, n // 2] += 2 * sr.GATE * n * sr.ULP * sr.norm1(a)
    assert sr.recon_t(torch.from_numpy(a.copy()), torch.from_numpy(q), torch.from_numpy(bad_t)) > sr.GATE
    z = torch.zeros((4, 4), dtype=torch.float64)
    assert sr.recon_t(z, torch.eye(4, dtype=torch.float64), z) == 0.0


@pytest.mark.parametrize("n", TRIDIAGONAL_ORDERS)
def test_lapack_on_the_tridiagonal_inputs(n):
    for name, (d, e) in sr.tridiagonal_inputs(n).items():
        t = sr.tridiagonal(d, e)
        w, z = np.linalg.eigh(t)
        figures = (sr.recon(t, z, np.diag(w)), sr.orth(z))
        print(f"[{name} n={n}] eigh(T) recon {figures[0]:.3f} orth {figures[1]:.3f}")
        assert max(figures) <= sr.LAPACK_GATE, (name, n, figures)
        if name == "toeplitz":
            err = np.abs(w - sr.toeplitz_exact(n)).max()
            assert err <= sr.LAPACK_GATE * n * sr.ULP * 4, (n, err)


def test_the_inputs_are_what_they_claim():
    n = 322
    t = sr.tridiagonal_inputs(n)
    assert all(len(d) == n and len(e) == n and e[-1] == 0.0 for d, e in t.values())
    assert np.all(t["torn"][1][2::3] == 0.0) and np.count_nonzero(t["torn"][1]) > n // 2
    assert np.all(t["negative"][1][:-1] < 0.0)
    assert t["graded"][0][0] / t["graded"][0][-1] == pytest.approx(1e15)
    assert np.all(t["equal"][0] == 1.0) and np.all(t["equal"][1][:-1] == 1e-9)
    assert t["glued1e-12"][1][20] == 1e-12 and t["glued1e-4"][1][41] == 1e-4
    names, mats = sr.mixed_batch(n)
    assert names == sr.MIXED and mats.shape == (len(names), n, n)
    assert all(np.array_equal(a, a.T) for a in mats)
    # band storage round trip: a band-64 matrix survives, entries beyond the band are reported
    a = mats[names.index("band64")]
    ab = np.zeros((n, sr.LDAB))
    for k in range(sr.BAND + 1):
        ab[:n - k, k] = np.diag(a, -k)
    assert np.array_equal(sr.band_matrix(ab), a) and sr.band_beyond(ab) == 0.0
    ab[5, sr.BAND + 1] = 1e-300
    assert sr.band_beyond(ab) == 1e-300


def test_zero_matrix_convention():
    z = np.zeros((4, 4))
    assert sr.recon(z, np.eye(4), z) == 0.0
    assert sr.recon(z, np.eye(4), 1e-300 * np.eye(4)) == np.inf


@pytest.mark.parametrize("n", [130, 256, 1030])
def test_planted_perturbations_fail_the_gate(n):
    """
    Errors orders of magnitude below the suite's max-abs gates must fail the ratios.  Q + 1e-13 G fails orth at every order
    (ratio ~ 570).  One entry of T changed by delta moves Q T Q^T by delta q q^T, whose 1-norm is at least delta
    (|q|_1 |q|_inf >= |q|_2^2 = 1) and for a random Q about 2.3 delta, so recon rises by 2.3 delta / (n ulp |A|_1):
    delta = 1e-12 |A|_1 gives 79 at n = 130, where it is asserted, but 41 at n = 256 and 10 at n = 1030 -- a single entry
    weighs less the larger the matrix is.  At every order the change that MUST fail by the bound above,
    delta = 2 GATE n ulp |A|_1 (5.8e-12 |A|_1 at n = 256, 2.3e-11 |A|_1 at n = 1030), is asserted to fail.
    """
    a = sr.random_sym(n)
    q, t = lapack_reduction(a)
    assert sr.orth(q) <= sr.LAPACK_GATE and sr.recon(a, q, t) <= sr.LAPACK_GATE
    g = np.random.RandomState(5).randn(n, n)
    bad_q = q + 1e-13 * g
    print(f"[n={n}] orth(Q + 1e-13 G) = {sr.orth(bad_q):.1f}")
    assert sr.orth(bad_q) > sr.GATE
    assert np.abs(bad_q @ bad_q.T - np.eye(n)).max() < 1e-11          # (the suite's max-abs gate does not see it)
    k = n // 2
    for what, delta in (("1e-12 |A|", 1e-12 * sr.norm1(a)), ("2 GATE n ulp |A|", 2 * sr.GATE * n * sr.ULP * sr.norm1(a))):
        bad_d, bad_e = t.copy(), t.copy()
        bad_d[k, k] += delta
        bad_e[k + 1, k] += delta
        bad_e[k, k + 1] = bad_e[k + 1, k]
        r_d, r_e = sr.recon(a, q, bad_d), sr.recon(a, q, bad_e)
        print(f"[n={n}] recon with d[{k}] / e[{k}] changed by {what}: {r_d:.1f} / {r_e:.1f}")
        if n == 130 or what != "1e-12 |A|":
            assert r_d > sr.GATE and r_e > sr.GATE, (n, what, r_d, r_e)
    w, v = np.linalg.eigh(a)
    bad_w = w.copy()
    bad_w[n // 3] += 2 * sr.GATE * n * sr.ULP * sr.norm1(a)
    assert sr.recon(a, v, np.diag(bad_w)) > sr.GATE
