"""
GPU tests of the pairwise comparison of mode subspaces (``k_mode_subspace`` of csrc/mode_subspace.hip) through its layers:
``DeviceBatchSolver.rmsip`` / ``covariance_overlap`` (``sc_dev_subspace_f64``), ``mode_overlap_matrix``
(``sc_dev_subspace_gram_f64``) and ``nma.rmsip`` / ``covariance_overlap`` / ``mode_overlap_matrix`` (``sc_modes_subspace``).

The model is tests/subspace.py evaluated on the solver's OWN (w, v): what is under test is the consumer -- which rows it
takes, which it never reads, which pair lands where -- and its arithmetic, gated by the derived bounds of that module
(``|G - np_gram| <= 2 m eps``, ``|S - np_S| <= 8 m eps t_a t_b``, RMSIP and the covariance overlap through those bounds
propagated; tests/test_subspace_host.py shows that the float64 model itself stays inside them).  Every comparison prints its
largest |difference| / bound.

Ensembles: one random cloud and small perturbations of it under ``InvariantForceField``.  Shapes: N = 7 ANM (m = 21, odd:
8-byte aligned rows, one partial chunk of 32 columns), N = 24 ANM (m = 72, several chunks, 66 non-trivial modes so that 65
listed rows cross the 64 tile), N = 67 ANM (m = 201, a chunk tail and several tiles), N = 33 GNM (dim 1); listed rows k in
{1, 3, 16, 17, 65}, where 16 / 17 also sit on either side of a 16-row MFMA block and k <= 32 takes the 32 tile; batches of
1, 2 and 5.  Bit-level statements compare an entry with the entry of the same two members on the same sides of the kernel:
in a self-comparison the member with the larger index is the first operand.
"""
import numpy as np
import pytest

from springcraft_amd import _hip
from springcraft_amd.batch import DeviceBatchSolver, _listed_pick, _rmsip_pick
from tests.subspace import (CUTOFF, EPS, cov_overlap_interval, cov_weights, ensemble, np_gram, np_S, pinv_rows,
                            rmsip_interval, s_bound)
from tests.test_batch_consumers_gpu import solved, window_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


_SOLVED = {}


def ensemble_of(sc, torch, n_atoms, batch, dim=3):
    """A finished full-spectrum solver of the ensemble at this shape with read-only host copies of (w, v): once per shape."""
    key = (n_atoms, batch, dim)
    if key not in _SOLVED:
        coords = ensemble(n_atoms, batch)
        s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF if dim == 3 else 10.0), dim=dim)
        for a in (coords, w, v):
            a.setflags(write=False)
        _SOLVED[key] = (s, coords, w, v)
    return _SOLVED[key]


def check_matrix(kind, got, w, v, rows, what, wb=None, vb=None, rows_b=None, listed=None, square=True):
    """
    ``got`` = (out, S, t_a, t_b) of ``_subspace_matrix(kind, ..., raw=True)`` on host against the model on (w, v)[, (wb, vb)]
    with per-member row lists ``rows`` / ``rows_b``: S inside its bound everywhere, t inside (k + 4) eps, the public
    quantity inside the propagated interval off the diagonal and inside the issue's gates on it.  ``listed``: rows the
    kernel was given per member when that is more than len(rows) (rows without weight add exactly nothing).
    """
    out, S, ta, tb = (np.asarray(x) for x in got)
    wb, vb, rows_b = (w, v, rows) if vb is None else (wb, vb, rows_b)
    m = v.shape[2]
    worst = 0.0
    for a in range(len(v)):
        for b in range(len(vb)):
            ra, rb = rows[a], rows_b[b]
            pa = cov_weights(w[a], ra) if kind == 1 else np.ones(len(ra))
            pb = cov_weights(wb[b], rb) if kind == 1 else np.ones(len(rb))
            # what the entry reports per member: the number of modes, or the trace of the covariance sum 1 / lambda = sum p^2
            T_a, T_b = ((pa ** 2).sum(), (pb ** 2).sum()) if kind == 1 else (pa.sum(), pb.sum())
            k = max(listed or 0, len(ra), len(rb), 1)
            assert abs(ta[a] - T_a) <= (k + 4) * EPS * T_a and abs(tb[b] - T_b) <= (k + 4) * EPS * T_b, (what, a, b)
            model = np_S(v[a], vb[b], ra, rb, pa, pb)
            bound = s_bound(m, pa.sum(), pb.sum())
            if bound == 0:
                # nothing selected on one side: S = 0; the RMSIP is 0 / 0, the covariance overlap 1 - sqrt(T / T) = 0 against a
                # member that has modes and 0 / 0 against another empty one
                assert S[a, b] == 0, (what, a, b)
                assert np.isnan(out[a, b]) if kind == 0 or T_a + T_b == 0 else out[a, b] == 0, (what, a, b, out[a, b])
                continue
            ratio = abs(S[a, b] - model) / bound
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, a, b, S[a, b], model, ratio)
            if square and a == b:
                if kind == 0:
                    assert abs(out[a, a] - 1) <= 1e-12, (what, a, out[a, a])
                else:
                    assert 1 - out[a, a] <= 1e-6, (what, a, out[a, a])
                continue
            lo, hi = rmsip_interval(model, T_a, T_b, bound) if kind == 0 else cov_overlap_interval(model, T_a, T_b, bound, k)
            assert lo <= out[a, b] <= hi, (what, a, b, lo, out[a, b], hi)
    print(f"{what}: max |S - model| / bound = {worst:.3e}")


def raw(s, kind, pick, other=None):
    return tuple(t.cpu().numpy() for t in s._subspace_matrix(kind, pick, other, raw=True))


# ---- 1. the shapes, the numbers of listed rows and the batch sizes ---------------------------------------------------------------
@pytest.mark.parametrize("n_atoms,dim,batch", [(7, 3, 5), (24, 3, 2), (67, 3, 2), (33, 1, 1), (24, 3, 5)])
def test_parity_inside_the_bounds(sc, torch, n_atoms, dim, batch):
    s, _, w, v = ensemble_of(sc, torch, n_atoms, batch, dim)
    m, ntriv = dim * n_atoms, 6 if dim == 3 else 1
    tag = f"N = {n_atoms} dim {dim} batch {batch}"
    pairs = [(a, b) for a in range(batch) for b in range(batch)]
    for k in [k for k in (1, 3, 16, 17, 65) if ntriv + k <= m]:
        rows = [np.arange(ntriv, ntriv + k)] * batch
        got = raw(s, 0, _rmsip_pick(k, None))
        check_matrix(0, got, w, v, rows, f"{tag} rmsip k = {k}")
        pub = s.rmsip(n_modes=k)
        assert pub.is_cuda and pub.dtype == torch.float64 and tuple(pub.shape) == (batch, batch)
        assert torch.equal(pub, pub.t()) and np.array_equal(pub.cpu().numpy(), got[0])       # symmetric bits, two calls agree
        assert torch.equal(s.rmsip(mode_subset=rows[0]), pub)
        cov = raw(s, 1, _listed_pick(rows[0], True))
        check_matrix(1, cov, w, v, rows, f"{tag} covariance overlap k = {k}")
        assert np.array_equal(cov[0], cov[0].T) and np.array_equal(s.covariance_overlap(rows[0]).cpu().numpy(), cov[0])
        g = s.mode_overlap_matrix(pairs, rows[0]).cpu().numpy()
        assert g.shape == (len(pairs), k, k)
        err = max(np.abs(g[i] - np_gram(v[a], v[b], rows[0], rows[0])).max() for i, (a, b) in enumerate(pairs))
        print(f"{tag} gram k = {k}: max |G - model| / (2 m eps) = {err / (2 * m * EPS):.3e}")
        assert err <= 2 * m * EPS
    # the covariance rule on the full spectrum, and the default of rmsip
    rule = [pinv_rows(w[b]) for b in range(batch)]
    assert all(np.array_equal(r, np.arange(ntriv, m)) for r in rule)
    check_matrix(1, raw(s, 1, _listed_pick(None, True)), w, v, rule, f"{tag} covariance overlap, covariance rule")
    k10 = min(10, m - ntriv)
    check_matrix(0, raw(s, 0, _rmsip_pick(10, None)), w, v, [np.arange(ntriv, ntriv + k10)] * batch, f"{tag} rmsip default")
    assert np.array_equal(s.rmsip().cpu().numpy(), raw(s, 0, _rmsip_pick(10, None))[0], equal_nan=True)


def test_a_row_listed_twice_counts_twice_and_nothing_listed_is_nan(sc, torch):
    s, _, w, v = ensemble_of(sc, torch, 24, 2)
    twice = [9, 7, 9]
    check_matrix(0, raw(s, 0, _rmsip_pick(10, twice)), w, v, [np.array(twice)] * 2, "modes [9, 7, 9]", square=False)
    g = s.mode_overlap_matrix([(1, 0)], twice).cpu().numpy()[0]
    assert np.abs(g - np_gram(v[1], v[0], twice, twice)).max() <= 2 * 72 * EPS and np.array_equal(g[0], g[2])
    out, S, ta, _ = raw(s, 0, _rmsip_pick(0, None))
    assert not S.any() and not ta.any() and np.isnan(out).all()
    assert tuple(s.mode_overlap_matrix([], twice).shape) == (0, 3, 3)
    assert tuple(s.mode_overlap_matrix([(0, 1)], []).shape) == (1, 0, 0)


def test_all_modes_of_two_complete_sets(sc, torch):
    """Unit weights on all m rows, trivial ones included: S = |V_a V_b^T|_F^2 = m for two orthonormal bases."""
    s, _, w, v = ensemble_of(sc, torch, 20, 2)

    def every_row(solver):
        sel = _hip.ModeSelection()
        sel.kind, sel.row0 = _hip.SC_SEL_FROM_ROW, 0
        return sel, None, None

    out, S, ta, tb = raw(s, 0, every_row)
    assert np.array_equal(ta, [60.0, 60.0])
    print(f"all 60 modes: max |S - m| / bound = {np.abs(S - 60).max() / s_bound(60, 60, 60):.3e}")
    assert np.abs(S - 60).max() <= s_bound(60, 60, 60) and np.abs(out - 1).max() <= 1e-12


# ---- 2. the solver's own selections ------------------------------------------------------------------------------------------------
def test_behind_an_index_range(sc, torch):
    coords = ensemble(24, 3)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF), subset_by_index=(3, 40))
    assert w.shape == (3, 38)
    check_matrix(0, raw(s, 0, _rmsip_pick(10, None)), w, v, [np.arange(3, 13)] * 3, "subset_by_index (3, 40): modes 6..15")
    check_matrix(1, raw(s, 1, _listed_pick(None, True)), w, v, [np.arange(3, 38)] * 3,
                 "subset_by_index (3, 40): covariance overlap over every non-trivial solved mode")
    check_matrix(0, raw(s, 0, _rmsip_pick(10, [7, 20, 12])), w, v, [np.array([4, 17, 9])] * 3, "modes [7, 20, 12]")
    with pytest.raises(ValueError, match="was not solved"):
        s.rmsip(mode_subset=[41])
    # against a full-spectrum solver of the same structures: the rectangle, the selection taken on each
    full, _, wf, vf = ensemble_of(sc, torch, 24, 2)
    got = raw(s, 0, _rmsip_pick(10, None), full)
    assert got[0].shape == (3, 2)
    check_matrix(0, got, w, v, [np.arange(3, 13)] * 3, "range solver against full solver", wb=wf, vb=vf,
                 rows_b=[np.arange(6, 16)] * 2, square=False)


def test_behind_a_value_window_counts_differ_and_one_is_empty(sc, torch):
    n_atoms, batch, K = 65, 5, 24
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, K, 3, batch=batch)
    assert expected.max() == K and expected.min() == 0 and len(set(expected)) >= 3
    s = DeviceBatchSolver(n_atoms, batch, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    first = s.rmsip()                                            # enqueued straight behind the solve
    s.finish()
    counts = s.counts.cpu().numpy()
    assert np.array_equal(counts, expected)
    for b in range(batch):
        s.v[b, counts[b]:] = float("nan")                        # what lies behind the count must not matter
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    rows = [np.arange(c) for c in counts]
    got = raw(s, 0, _rmsip_pick(10, None))
    assert np.array_equal(got[0], first.cpu().numpy(), equal_nan=True)
    check_matrix(0, got, w, v, rows, "window, rmsip", listed=K)
    check_matrix(1, raw(s, 1, _listed_pick(None, True)), w, v, rows, "window, covariance overlap", listed=K)
    empty = int(np.argmin(counts))
    nan = np.isnan(got[0])
    assert nan[empty].all() and nan[:, empty].all() and nan.sum() == 2 * batch - 1 and not got[1][empty].any()
    with pytest.raises(ValueError, match="subset_by_value"):
        s.rmsip(mode_subset=[7])


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_position_or_launch_shape(sc, torch):
    n_atoms = 24
    ff = sc.InvariantForceField(CUTOFF)
    s2, _, _, _ = ensemble_of(sc, torch, n_atoms, 2)
    s5, _, _ = solved(sc, torch, ensemble(n_atoms, 5, seed=3), ff)
    # the consumer's own property: the same eigenpairs as members (0, 1) of two and as members (1, 4) of five
    for dst, src in ((1, 0), (4, 1)):
        s5.w[dst].copy_(s2.w[src])
        s5.v[dst].copy_(s2.v[src])
    calls = [lambda s, o=None: s.rmsip(other=o), lambda s, o=None: s.rmsip(n_modes=65, other=o),
             lambda s, o=None: s.covariance_overlap(other=o), lambda s, o=None: s.covariance_overlap([7, 30, 8], other=o)]
    for call in calls:
        r2, r5 = call(s2), call(s5)
        assert bool(torch.isfinite(r5).all()) and torch.equal(r2, r2.t()) and torch.equal(r5, r5.t())
        assert torch.equal(r2, call(s2))                                         # two calls agree
        assert r5[4, 1].item() == r2[1, 0].item() and r5[4, 4].item() == r2[1, 1].item() and r5[1, 1].item() == r2[0, 0].item()
        assert r5[4, 2].item() != r2[1, 0].item()
        # the rectangle against another solver: (5, 2), its entry for the same two members on the same sides
        rect = call(s5, s2)
        assert tuple(rect.shape) == (5, 2)
        assert rect[4, 0].item() == r2[1, 0].item() and rect[4, 1].item() == r2[1, 1].item() and rect[1, 0].item() == r2[0, 0].item()
        assert torch.equal(rect, call(s5, s2))
    rows = np.arange(6, 23)
    t5, t2 = s5.mode_overlap_matrix([(4, 1), (0, 3)], rows), s2.mode_overlap_matrix([(1, 0)], rows)
    assert torch.equal(t5[0], t2[0]) and torch.equal(s5.mode_overlap_matrix([(4, 0)], rows, other=s2)[0], t2[0])
    # a weight-zero row is selected out, not multiplied by zero
    ref = s5.covariance_overlap()
    s5.v[2, 0:6] = float("nan")                                  # the trivial rows: under the covariance rule's threshold
    assert torch.equal(s5.covariance_overlap(), ref)


def test_a_non_finite_member_gives_nan_in_its_row_and_column_only(sc, torch):
    """
    A NaN coordinate under a force field without a cut-off reaches the member's Hessian (with a cut-off it would only
    isolate the atom: every comparison with NaN is false), the solver rejects that matrix and leaves NaN eigenvalues.
    """
    n_atoms, batch = 24, 3
    ff = sc.HinsenForceField()
    coords = ensemble(n_atoms, batch)

    def run(c):
        s = DeviceBatchSolver(n_atoms, batch, ff)
        s.solve(torch.from_numpy(np.ascontiguousarray(c)).cuda())
        return s, s.rmsip(), s.covariance_overlap(), s.rmsip(mode_subset=[7, 9, 30]), s.mode_overlap_matrix([(0, 2), (2, 1)], [7, 9])

    good, *ref = run(coords)
    good.finish()
    broken = coords.copy()
    broken[1, 5, 2] = np.nan
    bad, *got = run(broken)
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    for g, r in zip(got[:3], ref[:3]):
        nan = torch.isnan(g)
        assert bool(nan[1].all()) and bool(nan[:, 1].all()) and int(nan.sum()) == 2 * batch - 1
        for a, b in ((0, 0), (0, 2), (2, 0), (2, 2)):
            assert g[a, b].item() == r[a, b].item()
    assert torch.equal(got[3][0], ref[3][0]) and bool(torch.isnan(got[3][1]).all())


# ---- 4. the one-model functions --------------------------------------------------------------------------------------------------------
def test_the_one_model_functions_agree_with_the_model_and_the_batch(sc, torch):
    n_atoms = 24
    s, coords, w, v = ensemble_of(sc, torch, n_atoms, 2)
    ff = sc.InvariantForceField(CUTOFF)
    a, b = sc.ANM(coords[0], ff), sc.ANM(coords[1], ff)
    (wa, va), (wb, vb) = a.eigen(), b.eigen()
    m = 3 * n_atoms
    first, rule = np.arange(6, 16), np.arange(6, m)
    for got, kind, rows in ((sc.nma.rmsip(a, b), 0, first), (a.rmsip(b, mode_subset=[30, 7, 8]), 0, np.array([30, 7, 8])),
                            (sc.nma.covariance_overlap(a, b), 1, rule), (a.covariance_overlap(b, first), 1, first)):
        assert isinstance(got, float)
        pa, pb = (cov_weights(wa, rows), cov_weights(wb, rows)) if kind == 1 else (np.ones(len(rows)),) * 2
        Ta, Tb = ((pa ** 2).sum(), (pb ** 2).sum()) if kind == 1 else (pa.sum(), pb.sum())
        model, ds = np_S(va, vb, rows, rows, pa, pb), s_bound(m, pa.sum(), pb.sum())
        lo, hi = rmsip_interval(model, Ta, Tb, ds) if kind == 0 else cov_overlap_interval(model, Ta, Tb, ds, len(rows))
        assert lo <= got <= hi, (kind, rows, lo, got, hi)
    assert abs(sc.nma.rmsip(a, a) - 1) <= 1e-12 and 1 - sc.nma.covariance_overlap(b, b) <= 1e-6
    g = sc.nma.mode_overlap_matrix(a, b, first, [7, 9, 9])
    assert g.shape == (10, 3) and np.abs(g - np_gram(va, vb, first, [7, 9, 9])).max() <= 2 * m * EPS
    assert np.array_equal(a.mode_overlap_matrix(b, first), sc.nma.mode_overlap_matrix(a, b, first, first))
    assert sc.nma.mode_overlap_matrix(a, b, []).shape == (0, 0)
    # against the batch's entry for the same two structures.  Four solves of the same two matrices (two members, two solver
    # paths), each backward stable within 8 m eps |H| (the n-ulp ratios of the stage tests are below that); the projector on
    # the ten lowest non-trivial modes then moves by at most 2 * 8 m eps |H| / gap (Davis-Kahan), gap = lambda_16 -
    # lambda_15, RMSIP^2 = tr(P_a P_b) / 10 by the sum of the four, and the root of a value above 1 / 4 by as much again
    gap = min((x[16] - x[15]) / x[-1] for x in (w[0], w[1]))
    one, both = sc.nma.rmsip(a, b), s.rmsip()[1, 0].item()
    print(f"nma.rmsip {one!r} against the batch {both!r}: relative gap {gap:.3e}, bound {128 * m * EPS / gap:.3e}")
    assert both >= 0.5 and abs(one - both) <= 128 * m * EPS / gap
    with pytest.raises(IndexError):
        sc.nma.rmsip(a, b, mode_subset=[7, m])
    with pytest.raises(ValueError, match="10 and 24 atoms|24 and 10 atoms"):
        sc.nma.rmsip(a, sc.ANM(coords[0][:10], ff))
