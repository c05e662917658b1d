"""
The references of tests/partial_ratios.py checked on the CPU, on every input and range tests/test_partial_ratios_gpu.py
uses: LAPACK's dstebz + dstein (scipy.linalg.eigh_tridiagonal, lapack_driver="stebz") under the residual / orthogonality
ratios and against the exact eigenvalues; the exact eigenvalues against mpmath; the float64 restatement of k_stein +
CholQR2 (what the algorithm delivers, apart from the kernel); planted errors that must fail the gates; the window and
compaction rules against brute force.

Measured (n in 130, 257, 520, 1030 x nine inputs x lowest 70 / middle 44 / highest 65; profiles/partial_stage_ratios.txt):
  dstebz + dstein  resid <= 2.8, orth <= 2.2 except the top 65 of glued1e-12: resid 5.36 at n = 520 and 5.42 at n = 1030
                   (the glued Wilkinson cluster; both asserted at GATE), value <= 1.04
  restatement      resid <= 13.1, orth <= 0.08
  restatement with the run shift the kernel had before these tests (w[j] + place in the run x 10 eps |T|): the same except
                   glued1e-12 n = 520 top 65: resid 205;  graded n = 257 lowest 70: not finite -- that shift carries the
                   last members of a run whose members differ across the eigenvalues behind the run, two iterations then
                   converge to one vector, the Gram matrix is singular to working precision and the Cholesky floor
                   overflows.  The MI355X gave 202 and NaN (test_the_former_run_shift_fails_the_gate).
"""
import numpy as np
import pytest
import scipy.linalg

from tests import partial_ratios as pr
from tests import stage_ratios as sr

LD = pr.LD
needs_longdouble = pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here")

# dstebz + dstein above LAPACK_GATE (asserted at GATE): (input, n, range) -> measured resid
LAPACK_ABOVE = {("glued1e-12", 520, "top65"): 5.36, ("glued1e-12", 1030, "top65"): 5.42}


def cases(n):
    inputs = sr.tridiagonal_inputs(n)
    for name in sr.TRIDIAGONALS:
        d, e = inputs[name]
        for label, il, m in pr.ranges(n):
            yield name, label, il, m, d, e


def stebz(d, e, il, m):
    n = len(d)
    w, z = scipy.linalg.eigh_tridiagonal(d, e[:n - 1], select="i", select_range=(il, il + m - 1), lapack_driver="stebz")
    return w, z


@pytest.mark.parametrize("n", pr.ORDERS)
def test_lapack_stays_below_its_gate(n):
    failures = []
    for name, label, il, m, d, e in cases(n):
        w, z = stebz(d, e, il, m)
        r, o = pr.resid(d, e, w, z), pr.orth(z)
        print(f"[dstebz + dstein n={n}] {name:<11s} {label} resid {r:.3f} orth {o:.3f}")
        gate = sr.GATE if (name, n, label) in LAPACK_ABOVE else sr.LAPACK_GATE
        if not (r <= gate and o <= gate):
            failures.append((name, label, r, o))
    assert not failures, failures


@needs_longdouble
@pytest.mark.parametrize("n", pr.ORDERS)
def test_dstebz_values_against_exact_bisection(n):
    worst = {}
    for name, label, il, m, d, e in cases(n):
        w, _ = stebz(d, e, il, m)
        v = pr.value(w, pr.exact_eigenvalues(d, e, il, m), pr.t_norm1(d, e))
        worst[name] = max(worst.get(name, 0.0), v)
    print(f"[dstebz value n={n}] " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= pr.DSTEBZ_VALUE[k] for k, v in worst.items()), worst


@needs_longdouble
def test_exact_bisection_against_mpmath():
    """Every eigenvalue of four inputs at n = 130 lies within 2^-60 |T| of the true one: the Sturm count at 40 digits is
    at most k below lam - delta and above k at lam + delta."""
    import mpmath

    n = 130
    inputs = sr.tridiagonal_inputs(n)
    with mpmath.workdps(40):
        for name in ("toeplitz", "glued1e-12", "graded", "torn"):
            d, e = inputs[name]
            lam = pr.exact_eigenvalues(d, e, 0, n)
            delta = mpmath.mpf(pr.t_norm1(d, e)) * mpmath.mpf(2) ** -60
            md = [mpmath.mpf(float(x)) for x in d]
            me2 = [mpmath.mpf(float(x)) ** 2 for x in e[:n - 1]]

            def count(x):
                c, q = 0, md[0] - x
                c += q < 0
                for i in range(1, n):
                    q = md[i] - x - (me2[i - 1] / q if me2[i - 1] != 0 else 0)
                    c += q < 0
                return c

            for k in range(n):
                # (a long double as an exact mpf: two float64 pieces)
                x = mpmath.mpf(float(lam[k])) + mpmath.mpf(float(lam[k] - LD(float(lam[k]))))
                assert count(x - delta) <= k < count(x + delta), (name, k)
    t = pr.toeplitz_exact_ld(n)
    d, e = inputs["toeplitz"]
    assert np.abs(pr.exact_eigenvalues(d, e, 0, n) - t).max() <= 4.0 * 2.0 ** -60


@pytest.mark.parametrize("n", pr.ORDERS)
def test_restatement_of_the_algorithm(n):
    """k_stein + CholQR2 in float64 NumPy from dstebz's eigenvalues: below GATE on every case."""
    failures = []
    for name, label, il, m, d, e in cases(n):
        w, _ = stebz(d, e, il, m)
        z = pr.stein_restated(d, e, w)
        r, o = pr.resid(d, e, w, z), pr.orth(z)
        print(f"[restatement n={n}] {name:<11s} {label} resid {r:.3f} orth {o:.3f}")
        if not (r <= sr.GATE and o <= sr.GATE):
            failures.append((name, label, r, o))
    assert not failures, failures


def test_the_former_run_shift_fails_the_gate():
    """The two cases that exposed it, restated with the additive shift and with the kernel's present rule."""
    for name, n, il, m in (("glued1e-12", 520, 455, 65), ("graded", 257, 0, 70)):
        d, e = sr.tridiagonal_inputs(n)[name]
        w, _ = stebz(d, e, il, m)
        old = pr.stein_restated(d, e, w, shift_rule=pr.shifts_additive)
        new = pr.stein_restated(d, e, w)
        r_old, r_new = pr.resid(d, e, w, old), pr.resid(d, e, w, new)
        print(f"[{name} n={n} [{il}, {il + m})] resid with the additive shift {r_old:.3g}, with the monotone shift {r_new:.3g}")
        assert not r_old <= sr.GATE and r_new <= sr.GATE and pr.orth(new) <= sr.GATE


@pytest.mark.parametrize("il,m", [(0, 100), (100, 120)])
def test_multiplicities_behind_a_reduction(il, m):
    """Exact multiplicities behind an orthogonal reduction (an unreduced T): the model passes.  Without the separation of
    the shifts it is printed, not asserted: resid 8.9e4 / 940 with one LAPACK build, 9.9 / 3.0 with another -- whether the
    clusters' vectors collapse depends on the last bits of the reduction and of the eigenvalues."""
    d, e = pr.reduced_multiplicities()
    w, _ = stebz(d, e, il, m)
    z, bare = pr.stein_restated(d, e, w), pr.stein_restated(d, e, w, shift_rule=pr.shifts_none)
    r, r_bare = pr.resid(d, e, w, z), pr.resid(d, e, w, bare)
    print(f"[multiplicities [{il}, {il + m})] resid {r:.3g}, orth {pr.orth(z):.3g}; without the shift resid {r_bare:.3g}")
    assert r <= sr.GATE and pr.orth(z) <= sr.GATE


@pytest.mark.parametrize("n", [130, 520])
def test_planted_errors_fail_the_gates(n):
    """Into a correct (w, Z) of the top 65 of the Toeplitz matrix: one eigenvalue moved by 100 n ulp |T|, one vector entry
    changed by 1e-12, two vectors swapped, one vector replaced by its neighbour."""
    d, e = sr.tridiagonal_inputs(n)["toeplitz"]
    il, m = n - 65, 65
    w, z = stebz(d, e, il, m)
    tn = pr.t_norm1(d, e)
    assert pr.resid(d, e, w, z) <= sr.LAPACK_GATE and pr.orth(z) <= sr.LAPACK_GATE
    bad_w = w.copy()
    bad_w[20] += 100.0 * n * sr.ULP * tn
    r = pr.resid(d, e, bad_w, z)
    print(f"[n={n}] eigenvalue moved by 100 n ulp |T|: resid {r:.1f}")
    assert r > sr.GATE
    if pr.HAVE_LONGDOUBLE:
        assert pr.value(bad_w, pr.exact_eigenvalues(d, e, il, m), tn) > 3.0 * pr.DSTEBZ_VALUE["toeplitz"] * n
    # One entry of column j changed by delta adds delta (T - w_j) e_i to the residual, whose 1-norm is delta (|2 - w_j| + 2)
    # >= 2 delta: resid rises by at least delta / (2 n ulp).  1e-12 gives 17 at least at n = 130 (resid 29, orth 182 measured: asserted),
    # but only 4.3 at n = 520 -- a single entry weighs less the larger the matrix is; the change that MUST fail by that
    # bound, delta = 4 GATE n ulp (2.3e-11 at n = 520), is asserted at every order.
    for what, delta in (("1e-12", 1e-12), ("4 GATE n ulp", 4.0 * sr.GATE * n * sr.ULP)):
        bad_z = z.copy()
        bad_z[n // 2, 30] += delta
        r, o = pr.resid(d, e, w, bad_z), pr.orth(bad_z)
        print(f"[n={n}] one entry changed by {what}: resid {r:.1f} orth {o:.1f}")
        if n == 130 or what != "1e-12":
            assert max(r, o) > sr.GATE
        assert np.abs(bad_z.T @ bad_z - np.eye(m)).max() < 1e-10          # (a max-abs gate of 1e-10 does not see it)
    swapped = z.copy()
    swapped[:, [10, 11]] = swapped[:, [11, 10]]
    r = pr.resid(d, e, w, swapped)
    print(f"[n={n}] two vectors swapped: resid {r:.3g}")
    assert r > sr.GATE
    twice = z.copy()
    twice[:, 40] = twice[:, 41]
    r, o = pr.resid(d, e, w, twice), pr.orth(twice)
    print(f"[n={n}] a vector replaced by its neighbour: resid {r:.3g} orth {o:.3g}")
    assert r > sr.GATE and o > sr.GATE


def test_window_rule_against_brute_force():
    rs = np.random.RandomState(2)
    lam = np.arange(40, dtype=float)
    for _ in range(300):
        vl, vu = np.sort(rs.choice(np.concatenate([np.arange(-3, 44) * 1.0, np.arange(-3, 44) + 0.5, [-np.inf, np.inf]]),
                                   2, replace=False))
        own = int(rs.choice([40, 36, 30]))
        K = int(rs.randint(1, own + 1))
        il, count, start = pr.window_rule(lam, vl, vu, K, 1.0, None if own == 40 else own)
        inside = [k for k in range(own) if vl < lam[k] <= vu]
        assert il == sum(1 for x in lam if x <= vl)
        assert count == len(inside) and (not inside or inside[0] == il)
        assert 0 <= start <= own - K and (il >= own - K or start == il)
        w, z = pr.compact_rule(il, count, start, K, lam[start:start + K], np.eye(40)[start:start + K])
        keep = [k for k in inside if k < start + K][:K]
        assert np.array_equal(w[:len(keep)], lam[keep]) and np.all(np.isnan(w[len(keep):]))
        assert np.array_equal(z[:len(keep)], np.eye(40)[keep]) and not np.any(z[len(keep):])
    # the scale factor, exact and overflowing
    assert pr.window_rule(lam, 5.0 * 2.0 ** -400, 12.0 * 2.0 ** -400, 9, 2.0 ** 400) == (6, 7, 6)
    assert pr.window_rule(lam, 5.0 * 2.0 ** -1000, 1e10, 9, 2.0 ** 1000) == (6, 34, 6)
    assert pr.window_rule(lam, -1e10, 12.0 * 2.0 ** -1000, 9, 2.0 ** 1000) == (0, 13, 0)
    assert pr.window_rule(lam, 1e10, 1e20, 9, 2.0 ** 1000) == (40, 0, 31)


def test_small_orders_have_inputs():
    for n in (1, 2, 3, 20):
        t = sr.tridiagonal_inputs(n)
        assert all(len(d) == n and len(e) == n and e[-1] == 0.0 for d, e in t.values())
