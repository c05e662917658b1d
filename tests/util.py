"""Shared helpers for the test-suite (fixture loading, eigen-comparison metrics)."""
from os.path import abspath, dirname, join

import numpy as np

GOLDEN = join(dirname(abspath(__file__)), "golden")


def ref_data(name):
    """A data fixture copied from the reference's tests/data (CSV, maybe gzipped)."""
    return join(GOLDEN, "ref_data", name)


def load_csv(name, **kw):
    kw.setdefault("delimiter", ",")
    return np.genfromtxt(ref_data(name), **kw)


def generated(name):
    """A vector file written by oracle/make_golden.py (reference imported in the build container)."""
    return np.load(join(GOLDEN, "generated", name))


def structures():
    return generated("structures.npz")


def synthetic_coord(n, seed, box=None):
    # the reference's own generator (tests/test_interaction.py:80-84)
    if box is None:
        box = 5.0 * n ** (1.0 / 3.0)
    rs = np.random.RandomState(seed)
    return rs.rand(n, 3) * box


def forced_two_stage():
    """None, or the tridiagonalisation path forced through SPRINGCRAFT_TWO_STAGE (tools/test_matrix.sh): False / True."""
    import os

    e = os.environ.get("SPRINGCRAFT_TWO_STAGE")
    return None if e is None or e == "" else e != "0"


def oracle_patched(base_ff, natoms, contact_shutdown=None, contact_pair_off=None, contact_pair_on=None,
                   force_constants=None):
    """
    Oracle force field for ``PatchedForceField(base, ...)``: forcefield.py:183-226 restated on top of an oracle base force
    field (the restatement tests/test_oracle_golden.py::test_generated_patched pins to reference-generated vectors); the
    contact patches themselves are applied by the oracle's ``adjacency`` (interaction.py:193-213).
    """
    from oracle import enm_oracle as orc

    cutoff = base_ff.cutoff_distance

    def gamma(i, j, d2):
        if cutoff is None:
            fc = base_ff.gamma(i, j, d2)
        else:
            fc = np.zeros(len(d2))
            m = d2 <= cutoff**2
            fc[m] = base_ff.gamma(i[m], j[m], d2[m])
        if contact_pair_on is not None:
            pm = np.full((natoms, natoms), -1.0)
            pi, pj = np.asarray(contact_pair_on).T
            pm[pi, pj] = force_constants
            pm[pj, pi] = force_constants
            p = pm[i, j]
            fc = np.where(p == -1, fc, p)
        return fc

    return orc.OracleFF(gamma, cutoff, contact_shutdown=contact_shutdown, contact_pair_off=contact_pair_off,
                        contact_pair_on=contact_pair_on)


def pair_digest(pairs):
    import hashlib

    p = np.ascontiguousarray(np.asarray(pairs).astype(np.int64))
    return hashlib.sha256(p.tobytes()).hexdigest()


def check_eigenvalues(w, w_ref, n_trivial, rtol=1e-5):
    """
    SURVEY.md section 8(d) gates: relative 1e-5 on non-trivial modes, absolute
    1e-9 * lambda_max on the trivial (rigid-body) ones.
    """
    w = np.asarray(w)
    w_ref = np.asarray(w_ref)
    assert w.shape == w_ref.shape
    lam_max = np.abs(w_ref).max()
    assert np.all(np.abs(w[:n_trivial]) <= 1e-9 * lam_max), np.abs(w[:n_trivial]).max() / lam_max
    nt = slice(n_trivial, None)
    rel = np.abs(w[nt] - w_ref[nt]) / np.abs(w_ref[nt])
    assert rel.max() <= rtol, rel.max()
    assert np.all(np.diff(w) >= -1e-12 * lam_max), "eigenvalues not ascending"


def device_checks(torch, h, w, v, scale=None):
    """
    Residual (max column norm / lambda_max) and orthogonality of the eigenpairs (w, v) of one matrix, on the device.
    ``scale``: lambda_max of the whole spectrum when (w, v) is only part of it (default: max |w|).
    """
    r = h @ v.T - v.T * w[None, :]
    res = float(torch.linalg.vector_norm(r, dim=0).max() / (w.abs().max() if scale is None else scale))
    del r
    eye = torch.eye(len(w), dtype=torch.float64, device=w.device)
    orth = float((v @ v.T - eye).abs().max())
    return res, orth


def check_eigenvectors(a, w, v, tol_res=1e-5, tol_orth=1e-8):
    """Residual ||A v - lambda v|| <= tol * ||A|| and ||V V^T - I||_max <= tol_orth (rows = modes)."""
    a = np.asarray(a)
    norm_a = np.linalg.norm(a, 2) if a.shape[0] <= 2048 else np.abs(w).max()
    r = a @ v.T - v.T * w[None, :]
    res = np.linalg.norm(r, axis=0).max() / norm_a
    assert res <= tol_res, res
    g = v @ v.T
    orth = np.abs(g - np.eye(len(w))).max()
    assert orth <= tol_orth, orth
    return res, orth


def subspace_error(a, w_ref, v_ref, lo, hi, v, res_fro, cluster_gap=1e-3):
    """
    Subspace check of the eigenvectors v (rows) of the eigenvalues lo..hi of the symmetric matrix `a`, against the
    reference eigenpairs (w_ref ascending, v_ref columns): the sine of the largest angle between v and the reference's
    invariant subspace of the clusters (split at gaps >= cluster_gap lambda_max) that [lo, hi] touches, with its
    Davis-Kahan bound 2 (||R||_F + ||R_ref||_F) / gap (res_fro = ||R||_F of v).  When the range holds whole clusters this
    is ||P - P_ref||_2; when lo / hi cut a cluster, ||(I - P_cluster) v||.  Returns (error, bound, (first, last) index
    of the clusters).
    """
    n = len(w_ref)
    scale = np.abs(w_ref).max()
    delta = cluster_gap * scale
    a0, b0 = lo, hi
    while a0 > 0 and w_ref[a0] - w_ref[a0 - 1] < delta:
        a0 -= 1
    while b0 < n - 1 and w_ref[b0 + 1] - w_ref[b0] < delta:
        b0 += 1
    gap = np.inf
    if a0 > 0:
        gap = min(gap, w_ref[a0] - w_ref[a0 - 1])
    if b0 < n - 1:
        gap = min(gap, w_ref[b0 + 1] - w_ref[b0])
    u = v_ref[:, a0:b0 + 1]
    r_ref = np.linalg.norm(a @ u - u * w_ref[a0:b0 + 1][None, :])
    d = v.T - u @ (u.T @ v.T)
    err = np.linalg.norm(d, 2) if d.size else 0.0
    bound = 2.0 * (res_fro + r_ref) / gap if np.isfinite(gap) else 0.0
    return err, max(bound, 1e-13), (a0, b0)


# ---- matrices with known spectra ------------------------------------------------------------------------------
# Elastic networks on a cubic lattice (spacing 3.8 A, cutoff 4.5 A: only axis neighbours are in contact) have the
# spectra of sums of path graphs (tests/test_large_order_gpu.py explains the closed forms).
LATTICE_SPACING, LATTICE_CUTOFF = 3.8, 4.5


def rotation(seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def lattice(a, b, c, seed):
    """a x b x c grid points (index order i, j, k), spacing 3.8 A, rotated and shifted."""
    g = np.stack(np.meshgrid(np.arange(a), np.arange(b), np.arange(c), indexing="ij"), -1).reshape(-1, 3)
    return g * LATTICE_SPACING @ rotation(seed).T + np.array([12.5, -7.25, 3.0])


def path_eigs(m):
    return 4.0 * np.sin(np.pi * np.arange(m) / (2.0 * m)) ** 2


def gnm_exact(a, b, c):
    pa, pb, pc = (path_eigs(m).astype(np.longdouble) for m in (a, b, c))
    return (pa[:, None, None] + pb[None, :, None] + pc[None, None, :]).ravel()


def anm_exact(a, b, c):
    return np.concatenate([np.repeat(path_eigs(a), b * c), np.repeat(path_eigs(b), a * c),
                           np.repeat(path_eigs(c), a * b)])


def glued_wilkinson(blocks, glue, order=21):
    """
    (d, e) of `blocks` Wilkinson matrices W_order^+ (d_i = |i - (order - 1) / 2|, e_i = 1) glued by off-diagonal
    entries `glue`: every eigenvalue of W^+ becomes a cluster of `blocks` eigenvalues spread by ~glue, and the top pairs
    of W^+ (already equal to ~1e-14) clusters of 2 * blocks.
    """
    d0 = np.abs(np.arange(order) - (order - 1) / 2.0)
    d = np.tile(d0, blocks)
    e = np.ones(blocks * order - 1)
    e[order - 1::order] = glue
    return d, e


def tridiagonal(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def signed_permutation(seed, n):
    """An exact orthogonal similarity: P A P^T with P a random permutation with random signs."""
    rs = np.random.RandomState(seed)
    return rs.permutation(n), rs.choice([-1.0, 1.0], n)


def permute(a, perm, signs):
    return (a * signs[:, None] * signs[None, :])[np.ix_(perm, perm)]


def clustered_spectrum(rel_spacing, sizes=(1, 5, 12, 1, 8, 3, 20, 1, 7, 2), seed=0, n=None):
    """
    Eigenvalues in clusters: cluster c of `sizes[c]` members at centre mu_c (mu_c spread over [-3, 5], well apart) with
    members mu_c (1 + k rel_spacing), k = 0 .. size - 1 (rel_spacing 0: exact multiplicities), then simple eigenvalues up
    to order `n` filling the gaps between the centres.
    """
    rs = np.random.RandomState(seed)
    centres = np.linspace(-3.0, 5.0, len(sizes)) + 0.01
    w = [mu * (1.0 + rel_spacing * np.arange(s)) for mu, s in zip(centres, sizes)]
    k = sum(sizes)
    if n is not None and n > k:
        fill = rs.uniform(-3.5, 5.5, n - k)
        # keep the simple eigenvalues 0.05 away from every cluster centre
        for mu in centres:
            fill = np.where(np.abs(fill - mu) < 0.05, fill + 0.1, fill)
        w.append(fill)
    return np.sort(np.concatenate(w))


def random_orthogonal(seed, n):
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(n, n))
    return q * np.sign(np.diag(r))


def _largest_lattice(n):
    """(a, a, c) with a = floor(cbrt(n)) and c = n // a**2: a near-cubic grid of at most n points."""
    a = 1
    while (a + 1) ** 3 <= n:
        a += 1
    return a, a, n // (a * a)


def degenerate_members(n, seed, names=None):
    """
    The matrices at which eigensolvers go wrong, all of order `n`, for batched solves with mixed members
    (tests/test_batched_degenerate_gpu.py; tests/test_batched_degenerate_host.py checks the constructions themselves).
    Returns (members, exact): `members` a list of (name, a) in the fixed order below, every `a` exactly symmetric float64;
    `exact` maps the names whose spectrum is known in closed form to it (ascending).  `names`: build only these (a member
    is the same matrix whichever others are built with it: each draws from a random stream of its own).

    random          randn + randn^T, the control
    identity, zero  as named
    diag            diagonal, random entries
    tridiag         already tridiagonal
    band40/64/65    random with half-width 40 (inside the stage-1 band of 64), exactly 64, and 65 (one diagonal outside)
    blockdiag       two dense random blocks of orders n // 2 + 5 and the rest with exact zeros between them: the
                    tridiagonal matrix splits at a position that is no multiple of 64
    rank1           I + 5 q q^T
    clustered       Q diag(clustered_spectrum(0)) Q^T: exact multiplicities (exact up to the rounding of the product)
    nearclustered   the same with members 1e-13 (relative) apart: clustered but not deflated
    graded          Q diag(logspace(-12, 3, n)) Q^T
    gluedW          n // 21 Wilkinson blocks W21+ glued by 1e-10, embedded in 30 I, under a signed permutation
    big, small      random * 1e150, random * 1e-150
    kirchhoff       GNM Kirchhoff matrix of the largest near-cubic lattice with at most n atoms (integer entries, exact
                    multiplicities, spectrum gnm_exact < 12), padded by the diagonal 13, 14, ...
    """
    order = ["random", "identity", "zero", "diag", "tridiag", "band40", "band64", "band65", "blockdiag", "rank1",
             "clustered", "nearclustered", "graded", "gluedW", "big", "small", "kirchhoff"]
    wanted = order if names is None else list(names)
    assert set(wanted) <= set(order), sorted(set(wanted) - set(order))
    exact, cache = {}, {}

    def stream(name):
        return np.random.RandomState([seed, order.index(name)])

    def sym(a):
        return np.tril(a) + np.tril(a, -1).T

    def random():
        if "random" not in cache:
            g = stream("random").randn(n, n)
            cache["random"] = sym(g + g.T)
        return cache["random"]

    def q():
        if "q" not in cache:
            cache["q"] = random_orthogonal(seed + 1, n)
        return cache["q"]

    def band(name):
        i = np.arange(n)
        return np.where(np.abs(i[:, None] - i[None, :]) <= int(name[4:]), stream(name).randn(n, n), 0.0)

    def diag(name):
        d = stream(name).randn(n)
        exact[name] = np.sort(d)
        return np.diag(d)

    def tridiag(name):
        rs = stream(name)
        return tridiagonal(rs.randn(n), rs.randn(n - 1))

    def blockdiag(name):
        rs, n1 = stream(name), n // 2 + 5
        a = np.zeros((n, n))
        for lo, hi in ((0, n1), (n1, n)):
            g = rs.randn(hi - lo, hi - lo)
            a[lo:hi, lo:hi] = g + g.T
        return a

    def rank1(name):
        q0 = q()[:, 0]
        # (q0 is a unit vector to rounding: the one eigenvalue that is not 1 is 1 + 5 |q0|^2)
        exact[name] = np.concatenate([np.ones(n - 1), [1.0 + 5.0 * float(q0 @ q0)]])
        return np.eye(n) + 5.0 * np.outer(q0, q0)

    def clustered(name):
        lam = clustered_spectrum(0.0 if name == "clustered" else 1e-13, n=n)
        if name == "clustered":
            exact[name] = lam
        return (q() * lam) @ q().T

    def glued(name):
        nw = n // 21
        a = 30.0 * np.eye(n)
        a[:21 * nw, :21 * nw] = tridiagonal(*glued_wilkinson(nw, 1e-10))
        return permute(a, *signed_permutation(seed + 2, n))

    def kirchhoff(name):
        from oracle import enm_oracle as orc

        a, b, c = _largest_lattice(n)
        m = a * b * c
        pad = 13.0 + np.arange(n - m)
        k = np.diag(np.concatenate([np.zeros(m), pad]))
        k[:m, :m] = orc.compute_kirchhoff(lattice(a, b, c, seed), orc.invariant_ff(LATTICE_CUTOFF))[0]
        exact[name] = np.concatenate([np.sort(gnm_exact(a, b, c)).astype(np.float64), pad])
        return k

    def ones(name):
        exact[name] = np.ones(n) if name == "identity" else np.zeros(n)
        return np.eye(n) if name == "identity" else np.zeros((n, n))

    build = {"random": lambda name: random(), "identity": ones, "zero": ones, "diag": diag, "tridiag": tridiag,
             "band40": band, "band64": band, "band65": band, "blockdiag": blockdiag, "rank1": rank1, "clustered": clustered,
             "nearclustered": clustered, "graded": lambda name: (q() * np.logspace(-12, 3, n)) @ q().T, "gluedW": glued,
             "big": lambda name: random() * 1e150, "small": lambda name: random() * 1e-150, "kirchhoff": kirchhoff}
    members = [(name, sym(build[name](name))) for name in order if name in wanted]
    return members, exact
