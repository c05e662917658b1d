"""
Stage-level tests of the partial-spectrum solver (springcraft_amd/csrc/stein.hip) on chosen tridiagonal matrices, through
the staged debug entry sc_dbg_partial_tridiag_host (the product's host functions and kernels, nothing of its own):
k_sturm_range against exact eigenvalues in units of ulp |T|, k_stein + CholQR2 by dstein's residual and orthogonality
ratios in units of n ulp, k_window_count / k_window_compact bit for bit against their restated rules
(tests/partial_ratios.py).  The end-to-end tests reach these kernels only behind an orthogonal reduction and hold them to
max-abs gates several digits wider.  Every figure is printed before anything is asserted; profiles/partial_stage_ratios.txt
holds the figures of the first run beside LAPACK's and the restatement's (tests/test_partial_ratios_host.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import partial_ratios as pr
from tests import stage_ratios as sr

pytestmark = pytest.mark.gpu

NAMES = sr.TRIDIAGONALS
LD = pr.LD


@pytest.fixture(scope="module")
def lib_ctx():
    from springcraft_amd import _hip

    L = pr.debug_lib()
    ctx = _hip.Context(0)
    try:
        yield L, ctx
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def inputs(n):
    t = sr.tridiagonal_inputs(n)
    d = np.stack([t[k][0] for k in NAMES])
    e = np.stack([t[k][1] for k in NAMES])
    d.setflags(write=False)
    e.setflags(write=False)
    return d, e


@functools.lru_cache(maxsize=None)
def exact(n, b, il, m):
    d, e = inputs(n)
    lam = pr.exact_eigenvalues(d[b], e[b], il, m)
    lam.setflags(write=False)
    return lam


def value_bound(name):
    """3 x dstebz's worst value on the input, never tighter than 3 (the kernel's bracket stops at ulp max|Gershgorin| and
    the product-form count has one more rounding per row than the ratio form)."""
    return max(3.0, 3.0 * pr.DSTEBZ_VALUE.get(name, 1.0))


def check_values(label, name, d, e, w, lam, failures):
    """value <= the bound of the input, |w - lam| <= GATE n ulp |T|, w non-decreasing."""
    n = len(d)
    tn = pr.t_norm1(d, e)
    v = pr.value(w, lam, tn) if tn > 0.0 else float(np.abs(w).max())
    print(f"[{label}] {name:<11s} value {v:.3g} (bound {value_bound(name):.3g})")
    if not v <= value_bound(name):
        failures.append((label, name, "value", v))
    if not v / n <= sr.GATE:
        failures.append((label, name, "value / n", v / n))
    if not np.all(np.diff(w) >= 0.0):
        failures.append((label, name, "order"))


def check_vectors(label, name, d, e, w, z, failures, gate=sr.GATE):
    fig = {"resid": pr.resid(d, e, w, z), "orth": pr.orth(z)}
    print(f"[{label}] {name:<11s} " + "  ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    for k, v in fig.items():
        if not v <= gate:
            failures.append((label, name, k, v))
    return fig


# ---- values only: k_sturm_range ------------------------------------------------------------------------------------------
VALUE_RANGES = [(130, 0, 130), (257, 0, 257)] + [(1030, il, m) for _, il, m in pr.ranges(1030)]


@pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no exact reference")
@pytest.mark.parametrize("n,il,m", VALUE_RANGES)
def test_values_against_exact_bisection(lib_ctx, n, il, m):
    """All nine inputs in one batch, values only (stein_batched's d_x = nullptr return)."""
    L, ctx = lib_ctx
    d, e = inputs(n)
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=il, m=m, vectors=False)
    assert z is None
    failures = []
    for b, name in enumerate(NAMES):
        check_values(f"values n={n} [{il}, {il + m})", name, d[b], e[b], w[b], exact(n, b, il, m), failures)
    assert not failures, failures


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513])
def test_toeplitz_values_at_the_chunk_edges(lib_ctx, n):
    """The (1, 2, 1) Toeplitz matrix at the ends of the renormalisation period (4), the row chunks (64) and their groups
    (256), all indices, against 2 - 2 cos(k pi / (n + 1))."""
    L, ctx = lib_ctx
    d, e = np.full(n, 2.0), np.ones(n)
    e[-1] = 0.0
    w, _, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=n, vectors=False)
    failures = []
    check_values(f"toeplitz n={n}", "toeplitz", d, e, w[0], pr.toeplitz_exact_ld(n), failures)
    assert not failures, failures


@pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no exact reference")
@pytest.mark.parametrize("n", [130, 257])
def test_single_indices(lib_ctx, n):
    """m = 1 at both ends of the spectrum and next to them: an index off by one returns a neighbouring eigenvalue."""
    L, ctx = lib_ctx
    d, e = inputs(n)
    failures = []
    for il in (0, 1, n - 2, n - 1):
        w, _, _, _ = pr.partial_host(L, ctx, d, e, il=il, m=1, vectors=False)
        for b, name in enumerate(NAMES):
            check_values(f"single n={n} il={il}", name, d[b], e[b], w[b], exact(n, b, 0, n)[il:il + 1], failures)
    assert not failures, failures


def decoupled_cases():
    rs = np.random.RandomState(7)
    n = 70
    ints = np.concatenate([[0.0, 0.0], np.arange(1.0, n - 1)])
    d1 = ints[rs.permutation(n)]
    # a singular 2 x 2 block [[1, 1], [1, 1]] (eigenvalues 0, 2) in the middle of 1 x 1 blocks 3, 5, 7, ...
    d2 = np.concatenate([3.0 + 2.0 * np.arange(33), [1.0, 1.0], 3.0 + 2.0 * np.arange(33, 66)])
    e2 = np.zeros(len(d2))
    e2[33] = 1.0
    lam2 = np.sort(np.concatenate([[0.0, 2.0], 3.0 + 2.0 * np.arange(66)]))
    return [("integers", d1, np.zeros(n), np.sort(ints)), ("singular2x2", d2, e2, lam2)]


@pytest.mark.parametrize("case", range(2))
def test_exactly_decoupled_blocks(lib_ctx, case):
    """e = 0 everywhere (a double eigenvalue 0 among integers), and a singular 2 x 2 block among 1 x 1 blocks: the
    spectra are known exactly and every count meets exact zeros of the sequence."""
    L, ctx = lib_ctx
    name, d, e, lam = decoupled_cases()[case]
    n = len(d)
    failures = []
    w, _, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=n, vectors=False)
    check_values(f"decoupled {name}", name, d, e, w[0], lam.astype(LD), failures)
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=n)
    check_values(f"decoupled {name} (vectors)", name, d, e, w[0], lam.astype(LD), failures)
    check_vectors(f"decoupled {name}", name, d, e, w[0], z[0], failures)
    assert not failures, failures


# ---- vectors: k_stein + CholQR2 ------------------------------------------------------------------------------------------
VECTOR_RANGES = [(130, 0, 1), (130, 0, 63), (130, 66, 64), (130, 65, 65), (130, 1, 129), (130, 0, 130)] + \
    [(257, il, m) for _, il, m in pr.ranges(257)] + [(520, 520 - 65, 65)]


# The two cases that exposed k_stein's former run shift (w[j] + place in the run x 10 eps |T|; profiles/partial_stage_ratios.txt):
# the top 65 of glued1e-12 at n = 520 had resid 202, the lowest 70 of graded at n = 257 came back as NaN.  Both are held to
# GATE with all the others below; the second has a test of its own as well.
@pytest.mark.parametrize("n,il,m", VECTOR_RANGES)
def test_vectors_on_the_tridiagonal_inputs(lib_ctx, n, il, m):
    """resid and orth of all nine inputs (one batch): m at the 64-lane workgroup edges and the full spectrum at n = 130,
    the three ranges at n = 257, the top 65 at n = 520."""
    L, ctx = lib_ctx
    d, e = inputs(n)
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=il, m=m)
    failures = []
    for b, name in enumerate(NAMES):
        check_vectors(f"vectors n={n} [{il}, {il + m})", name, d[b], e[b], w[b], z[b], failures)
    assert not failures, failures


def test_graded_lowest_seventy(lib_ctx):
    """The lowest 70 eigenpairs of the matrix graded down to eps |T| at n = 257, alone: about 25 of the eigenvalues lie
    within 10 eps |T| of their predecessor without being equal.  (NaN vectors with the former run shift: it carried those
    members across the eigenvalues behind the run, two iterations converged to one vector, the Gram matrix was singular to
    working precision and k_chol_inv's 1e-300 floor overflowed.)  dstebz + dstein: resid 0.006, orth 0.03."""
    L, ctx = lib_ctx
    name, n, il, m = "graded", 257, 0, 70
    b = NAMES.index(name)
    d, e = inputs(n)
    w, z, _, _ = pr.partial_host(L, ctx, d[b], e[b], il=il, m=m)
    failures = []
    check_vectors(f"vectors n={n} [{il}, {il + m})", name, d[b], e[b], w[0], z[0], failures)
    assert not failures, failures


def test_vectors_with_split_gram(lib_ctx):
    """n = 1030: splits = 2, k_chol_inv sums two Gram slices; the top 65 of toeplitz and glued1e-4."""
    L, ctx = lib_ctx
    n, m = 1030, 65
    pick = [NAMES.index("toeplitz"), NAMES.index("glued1e-4")]
    d, e = inputs(n)
    w, z, _, _ = pr.partial_host(L, ctx, d[pick], e[pick], il=n - m, m=m)
    failures = []
    for k, b in enumerate(pick):
        check_vectors(f"vectors n={n} top {m}", NAMES[b], d[b], e[b], w[k], z[k], failures)
    assert not failures, failures


@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 24, 25, 28, 29, 32, 33])
def test_vectors_at_the_chunk_ends(lib_ctx, n):
    """Orders at the ends of the chunks of the factorisation (24 rows), the forward (28) and backward (20) passes and the
    rescale (32), m = min(n, 5) from the bottom and from the top."""
    L, ctx = lib_ctx
    d, e = inputs(n)
    m = min(n, 5)
    failures = []
    for il in sorted({0, n - m}):
        w, z, _, _ = pr.partial_host(L, ctx, d, e, il=il, m=m)
        for b, name in enumerate(NAMES):
            check_vectors(f"small n={n} il={il}", name, d[b], e[b], w[b], z[b], failures)
    assert not failures, failures


@pytest.mark.parametrize("n,m,members", [(65, 3, ["toeplitz", "glued1e-4", "negative"]),
                                         (130, 7, ["toeplitz", "wilkinson", "glued1e-12", "torn", "negative"])])
def test_batch_members_do_not_see_each_other(lib_ctx, n, m, members):
    """n m odd (65 x 3: stein_nm4 pads the records of members >= 1) and five different members: every member's bits are
    those of solving it alone."""
    L, ctx = lib_ctx
    pick = [NAMES.index(k) for k in members]
    d, e = inputs(n)
    il = (n - m) // 2
    w, z, _, _ = pr.partial_host(L, ctx, d[pick], e[pick], il=il, m=m)
    failures = []
    for k, b in enumerate(pick):
        w1, z1, _, _ = pr.partial_host(L, ctx, d[b], e[b], il=il, m=m)
        assert np.array_equal(w[k], w1[0]) and np.array_equal(z[k], z1[0]), (NAMES[b], "differs from the single solve")
        check_vectors(f"batch n={n} m={m}", NAMES[b], d[b], e[b], w[k], z[k], failures)
    assert not failures, failures


# ---- clusters --------------------------------------------------------------------------------------------------------------
def test_six_equal_eigenvalues(lib_ctx):
    """Six exact zeros on the diagonal between two Toeplitz blocks (all of whose eigenvalues are positive), e = 0 around
    them: the six vectors of the run must span e_40 .. e_45 exactly (projector difference <= GATE n ulp)."""
    L, ctx = lib_ctx
    d = np.concatenate([np.full(40, 2.0), np.zeros(6), np.full(40, 2.0)])
    e = np.ones(len(d))
    e[39:46] = 0.0
    e[-1] = 0.0
    n, m = len(d), 10
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=m)
    failures = []
    check_vectors("six zeros", "six zeros", d, e, w[0], z[0], failures)
    assert np.all(np.abs(w[0][:6]) <= value_bound("") * sr.ULP * pr.t_norm1(d, e)), w[0][:6]
    proj = pr.projector_difference(z[0][:, :6], np.eye(n)[:, 40:46])
    print(f"[six zeros] projector difference / (n ulp) = {proj / (n * sr.ULP):.3g}")
    assert proj <= sr.GATE * n * sr.ULP, proj / (n * sr.ULP)
    assert not failures, failures


def test_run_of_thirty(lib_ctx):
    """Thirty eigenvalues within 5 eps |T| (1 on the diagonal, coupled by 1e-17) under a shifted Toeplitz block: the run
    shift moves its members apart by up to 300 eps |T|."""
    L, ctx = lib_ctx
    d = np.concatenate([np.ones(30), np.full(60, 5.0)])
    e = np.concatenate([np.full(29, 1e-17), [0.0], np.ones(60)])
    e[-1] = 0.0
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=40)
    assert np.ptp(w[0][:30]) <= 5.0 * sr.ULP * pr.t_norm1(d, e), np.ptp(w[0][:30])
    failures = []
    check_vectors("run of 30", "run30", d, e, w[0], z[0], failures)
    assert not failures, failures


@pytest.mark.parametrize("il,m", [(0, 100), (100, 120)])
def test_multiplicities_behind_a_reduction(lib_ctx, il, m):
    """The Householder tridiagonal form of Q diag(lambda) Q^T with exact multiplicities up to 20
    (pr.reduced_multiplicities): T is unreduced, so T - lam I has ONE small pivot for a whole cluster.  The model without
    the separation of the shifts reaches resid 8.9e4 here with one LAPACK build and 9.9 with another
    (tests/test_partial_ratios_host.py), and a kernel built without it passed this test on the MI355X: the case checks
    clusters behind a reduction, it does not pin the shift."""
    L, ctx = lib_ctx
    d, e = pr.reduced_multiplicities()
    w, z, _, _ = pr.partial_host(L, ctx, d, e, il=il, m=m)
    failures = []
    check_vectors(f"multiplicities n={len(d)} [{il}, {il + m})", "clustered", d, e, w[0], z[0], failures)
    assert not failures, failures


# ---- windows: k_window_count, k_window_compact -------------------------------------------------------------------------------
def window_matrices():
    """(name, d, e, ascending eigenvalues as float64 -- exact for the integer spectra)."""
    rs = np.random.RandomState(11)
    n = 40
    out = []
    for shift in (0.0, -7.0, 3.0):
        ints = np.arange(n) + shift
        out.append((f"integers{shift:+.0f}", ints[rs.permutation(n)], np.zeros(n), ints))
    e = np.ones(n)
    e[-1] = 0.0
    out.append(("toeplitz", np.full(n, 2.0), e, pr.toeplitz_exact_ld(n).astype(float)))
    return out


def check_window(L, ctx, label, d, e, lams, vl, vu, K, f=None, own=None, vectors=True):
    """One window call on a batch: records, counts and compacted rows against the rules and the index-range solve."""
    d, e = np.atleast_2d(d), np.atleast_2d(e)
    batch, n = d.shape
    w, z, win, count = pr.partial_host(L, ctx, d, e, window=(vl, vu, K), f=f, own=own, vectors=vectors)
    fs = np.broadcast_to(1.0 if f is None else f, (batch,))
    owns = [None] * batch if own is None else list(np.broadcast_to(own, (batch,)))
    for b in range(batch):
        il, cnt, start = pr.window_rule(lams[b], vl, vu, K, fs[b], owns[b])
        print(f"[window {label}] member {b}: (vl, vu] = ({vl:g}, {vu:g}] K={K} f={fs[b]:g} own={owns[b]}: record "
              f"{win[b].tolist()} count {count[b]}, rule il={il} count={cnt} start={start}")
        assert win[b].tolist() == [il, cnt, start, 0] and count[b] == cnt, (label, b, win[b], count[b], (il, cnt, start))
        wr, zr, _, _ = pr.partial_host(L, ctx, d[b], e[b], il=start, m=K, vectors=vectors)
        we, ze = pr.compact_rule(il, cnt, start, K, wr[0], None if zr is None else zr[0].T)
        assert np.array_equal(w[b], we, equal_nan=True), (label, b, "w", w[b], we)
        if vectors:
            assert np.array_equal(z[b].T, ze), (label, b, "z")
            keep = int(np.count_nonzero(~np.isnan(we)))
            assert keep == min(cnt, K) and not np.any(z[b].T[keep:]), (label, b, keep)


WINDOWS = [
    # vl, vu, K: bounds on eigenvalues (the <= rule), between them, infinite, beside the spectrum; count = 0, < K, = K, > K
    (5.0, 12.0, 7), (5.0, 12.0, 10), (5.0, 12.0, 3), (4.5, 12.5, 8), (4.5, 5.0, 4), (5.0, 5.5, 4), (-np.inf, 3.0, 6),
    (30.0, np.inf, 12), (-np.inf, np.inf, 40), (-np.inf, np.inf, 5), (-100.0, -50.0, 3), (100.0, 200.0, 3),
    (38.0, 39.0, 1), (-1.0, 0.0, 2), (36.5, 1e300, 5),
]


@pytest.mark.parametrize("vl,vu,K", WINDOWS)
def test_window_on_integer_spectra(lib_ctx, vl, vu, K):
    """Batch of three integer spectra (0..39, -7..32, 3..42 in shuffled order, e = 0): different counts per member."""
    L, ctx = lib_ctx
    mats = window_matrices()[:3]
    check_window(L, ctx, "integers", np.stack([m[1] for m in mats]), np.stack([m[2] for m in mats]), [m[3] for m in mats],
                 vl, vu, K)


def test_window_batch_of_four_with_toeplitz(lib_ctx):
    """Four members, the bounds between eigenvalues of the Toeplitz member; values only as well."""
    L, ctx = lib_ctx
    mats = window_matrices()
    d, e, lams = np.stack([m[1] for m in mats]), np.stack([m[2] for m in mats]), [m[3] for m in mats]
    for vl, vu, K in ((0.5, 3.25, 9), (-0.5, 0.0625, 4), (3.5, 50.0, 16)):
        check_window(L, ctx, "four", d, e, lams, vl, vu, K)
        check_window(L, ctx, "four, values", d, e, lams, vl, vu, K, vectors=False)


def test_window_without_the_optional_outputs(lib_ctx):
    """win_out and count_out are optional: the same slots come back without them."""
    L, ctx = lib_ctx
    _, d, e, _ = window_matrices()[0]
    d, e = np.ascontiguousarray(d[None]), np.ascontiguousarray(e[None])
    n, K = d.shape[1], 9
    w, z = np.full((1, K), -777.0), np.full((1, K, n), -777.0)
    p = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    ctx.check(L.sc_dbg_partial_tridiag_host(ctx.handle, p(d), p(e), None, None, n, 1, 1, 0, K, 4.5, 12.5, 1, p(w), p(z), None,
                                            None))
    w2, z2, _, _ = pr.partial_host(L, ctx, d, e, window=(4.5, 12.5, K))
    assert np.array_equal(w, w2, equal_nan=True) and np.array_equal(z.transpose(0, 2, 1), z2)


@pytest.mark.parametrize("f,vl,vu", [(2.0 ** -400, 5.0 * 2.0 ** 400, 12.0 * 2.0 ** 400),
                                     (2.0 ** 400, 5.0 * 2.0 ** -400, 12.0 * 2.0 ** -400),
                                     (2.0 ** 400, -np.inf, 12.5 * 2.0 ** -400),
                                     (2.0 ** 1000, 5.0 * 2.0 ** -1000, 1e10),          # vu f overflows: clamped, all above
                                     (2.0 ** 1000, -1e10, 12.0 * 2.0 ** -1000),        # vl f overflows below
                                     (2.0 ** 1000, 1e10, 1e20)])                       # both beyond: empty
def test_window_scale_factor(lib_ctx, f, vl, vu):
    """The bounds are multiplied by the matrix' power-of-two factor; a product beyond the doubles is clamped."""
    L, ctx = lib_ctx
    _, d, e, lam = window_matrices()[0]
    check_window(L, ctx, "scaled", d, e, [lam], vl, vu, 9, f=f)


@pytest.mark.parametrize("vl,vu,K", [(20.5, np.inf, 6), (-np.inf, np.inf, 30), (27.0, 35.0, 4), (50.0, 2000.0, 3),
                                     (-np.inf, 1500.0, 12)])
def test_window_own_orders(lib_ctx, vl, vu, K):
    """Padded slots as the ragged solver builds them: the own eigenvalues 0 .. own - 1, pad eigenvalues 1000.. above them;
    own = 30 and 36 of n = 40 and an unpadded member in one batch."""
    L, ctx = lib_ctx
    rs = np.random.RandomState(3)
    n, owns = 40, [30, 36, 40]
    ds, lams = [], []
    for own in owns:
        lam = np.concatenate([np.arange(own, dtype=float), 1000.0 + np.arange(n - own)])
        ds.append(np.concatenate([lam[:own][rs.permutation(own)], lam[own:]]))
        lams.append(lam)
    check_window(L, ctx, "own", np.stack(ds), np.zeros((3, n)), lams, vl, vu, K, own=owns)


# ---- the stage against the product ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_stage,n,lo,hi", [(False, 300, 0, 69), (True, 513, 230, 273)])
def test_stage_composes_to_the_product(lib_ctx, two_stage, n, lo, hi):
    """d, e, scale and Q of sc_dbg_reduce_host and (w, Z) of the staged entry on that T reproduce sc_dev_eigh_range_f64:
    eigenvalues to GATE n ulp lambda_max, |V - (Q Z)^T|_1 <= GATE n ulp."""
    import torch

    from springcraft_amd import _hip

    L, _ = lib_ctx
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(two_stage)
        a = sr.random_sym(n)
        m = hi - lo + 1
        ta = torch.from_numpy(a.copy()[None]).cuda()
        tw = torch.empty((1, m), dtype=torch.float64, device="cuda")
        tv = torch.empty((1, m, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.sc_dev_eigh_range_f64(ctx.handle, C.c_void_p(ta.data_ptr()), n, 1, lo, hi, C.c_void_p(tw.data_ptr()),
                                          C.c_void_p(tv.data_ptr())))
        ctx.synchronize()
        w, v = tw.cpu().numpy()[0], tv.cpu().numpy()[0]
        d, e, s, _, q, two = sr.reduce_host(L, ctx, a[None], sr.Q_ALL)
        assert two == two_stage
        ws, z, _, _ = pr.partial_host(L, ctx, d, e, il=lo, m=m)
    finally:
        ctx.close()
    diff = sr.norm1(v - (q[0] @ z[0]).T) / (n * sr.ULP)
    eig = np.abs(w - ws[0] / s[0]).max() / (np.abs(np.linalg.eigvalsh(a)).max() * n * sr.ULP)
    print(f"[compose two_stage={two_stage} n={n} [{lo}, {hi}]] |V - (Q Z)^T|_1 / (n ulp) = {diff:.3g}, eigenvalue "
          f"difference / (n ulp lambda_max) = {eig:.3g}")
    assert diff <= sr.GATE and eig <= sr.GATE, (diff, eig)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(lib_ctx):
    """Every argument the entry refuses is SC_ERR_INVALID_ARG, and the context solves normally afterwards."""
    L, ctx = lib_ctx
    n = 20
    d, e = inputs(n)
    d, e = d[:2], e[:2]
    bad = [dict(il=-1, m=3), dict(il=0, m=0), dict(il=0, m=n + 1), dict(il=n - 2, m=3), dict(il=n, m=1),
           dict(window=(0.0, 1.0, 0)), dict(window=(0.0, 1.0, n + 1)), dict(window=(1.0, 1.0, 3)),
           dict(window=(2.0, 1.0, 3)), dict(window=(np.nan, 1.0, 3)), dict(window=(0.0, np.nan, 3)),
           dict(window=(0.0, 1.0, 5), own=[4, n]), dict(window=(0.0, 1.0, 5), own=[n, n + 1])]
    for kw in bad:
        rc, _ = pr.partial_raw(L, ctx, d, e, **kw)
        assert rc == pr.SC_ERR_INVALID_ARG, (kw, rc)
    p = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    w, z = np.zeros((2, 3)), np.zeros((2, 3, n))
    dd, ee = np.ascontiguousarray(d), np.ascontiguousarray(e)

    def call(dp, ep, wp, zp, nn=n, batch=2, vectors=1):
        return L.sc_dbg_partial_tridiag_host(ctx.handle, dp, ep, None, None, nn, batch, 0, 0, 3, 0.0, 0.0, vectors, wp, zp,
                                             None, None)

    assert call(None, p(ee), p(w), p(z)) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), None, p(w), p(z)) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), None, p(z)) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), p(w), None) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), p(w), p(z), nn=0) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), p(w), p(z), nn=46001) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), p(w), p(z), batch=0) == pr.SC_ERR_INVALID_ARG
    assert L.sc_dbg_partial_tridiag_host(None, p(dd), p(ee), None, None, n, 2, 0, 0, 3, 0.0, 0.0, 1, p(w), p(z), None,
                                         None) == pr.SC_ERR_INVALID_ARG
    assert call(p(dd), p(ee), p(w), None, vectors=0) == 0       # (values only needs no z_out)
    wv, zv, _, _ = pr.partial_host(L, ctx, d, e, il=0, m=3)
    assert np.array_equal(wv, w)
    failures = []
    for b in range(2):
        check_vectors("after refusals", NAMES[b], d[b], e[b], wv[b], zv[b], failures)
    assert not failures, failures
