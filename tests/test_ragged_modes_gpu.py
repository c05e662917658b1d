"""
GPU tests of ``RaggedBatchSolver``'s partial spectrum (``subset_by_index``, ``subset_by_value``) and mode consumers
(``sc_batch_plan_eigh_*`` / ``sc_batch_plan_modes_*``): structures of different sizes, force fields and masses in padded
slots ``diag(M, D)`` of one batched solve.

References are the oracle's matrices with ``np.linalg.eigh`` and the two formulas of tests/test_batch_consumers_gpu.py
on eigenpairs.  Gates of the partial solves, per structure, are those of tests/test_partial_spectrum_gpu.py with the
slot's norm as the scale, because the solver sees ``diag(M, D)``: S = 4 x the structure's largest absolute row sum, the
upper end of the pad interval.  Eigenvalues within 1e-11 S and ascending, column residual <= 1e-10 S against the oracle
matrix, ||V V^T - I||_max <= 1e-10, pad columns <= 1e-13 (the bound of tests/test_ragged_gpu.py).  Consumer gates are
those of tests/test_batch_consumers_gpu.py.  Figures are printed before they are asserted (``pytest -s``).
"""
import numpy as np
import pytest

from oracle import enm_oracle as orc
from tests.test_batch_consumers_gpu import (K_B, N_A, check_dcc, check_dcc_norm, check_msf, np_dcc, np_msf, pinv_rows)
from tests.util import forced_two_stage, load_csv, oracle_patched, structures, synthetic_coord

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _packed(torch, coords):
    return torch.from_numpy(np.concatenate(coords).astype(np.float64)).cuda().contiguous()


def _solver(sizes, ffs, **kw):
    from springcraft_amd.batch import RaggedBatchSolver

    return RaggedBatchSolver(sizes, ffs, **kw)


def _slot_scale(mat):
    return 4.0 * np.abs(mat).sum(axis=1).max()


# ---- the mixed ANM batch of cases 4, 7 and 10: computed once, never modified -------------------------------------------------
MIXED_SIZES = (43, 50, 37, 64)


@pytest.fixture(scope="module")
def mixed(sc):
    """Invariant 13 A, Hinsen, a patched Invariant and a mass-weighted Hinsen: coordinates, force fields, oracle Hessians."""
    sizes = MIXED_SIZES
    coords = [synthetic_coord(n, 300 + k) for k, n in enumerate(sizes)]
    on = np.array([[2, 30], [5, 6]])
    patch = dict(contact_pair_off=np.array([[0, 1]]), contact_pair_on=on, force_constants=np.array([2.5, 0.5]))
    ffs = [sc.InvariantForceField(13.0), sc.HinsenForceField(13.0),
           sc.PatchedForceField(sc.InvariantForceField(13.0), **patch), sc.HinsenForceField(13.0)]
    oracles = [orc.invariant_ff(13.0), orc.hinsen_ff(13.0), oracle_patched(orc.invariant_ff(13.0), sizes[2], **patch),
               orc.hinsen_ff(13.0)]
    masses = [None, None, None, np.random.RandomState(5).uniform(1.0, 20.0, sizes[3])]
    mats = []
    for c, o, mass in zip(coords, oracles, masses):
        h, _ = orc.compute_hessian(c, o)
        mats.append(h if mass is None else h * orc.mass_weight_matrix(mass, 3))
    spectra = [np.linalg.eigvalsh(h) for h in mats]
    return dict(sizes=sizes, coords=coords, ffs=ffs, masses=masses, mats=mats, spectra=spectra)


def _check_rows(tag, mat, w_ref, rows_ref, wk, vk, pad, S):
    """The partial-spectrum gates for rows ``rows_ref`` (global indices) of one structure; returns the figures."""
    m = len(mat)
    assert wk.shape == (len(rows_ref),) and vk.shape == (len(rows_ref), m), (tag, wk.shape, vk.shape)
    eig = np.abs(wk - w_ref[rows_ref]).max() / S
    res = np.linalg.norm(mat @ vk.T - vk.T * wk[None, :], axis=0).max() / S
    orth = np.abs(vk @ vk.T - np.eye(len(wk))).max()
    print(f"{tag}: eig {eig:.2e} S, residual {res:.2e} S, orth {orth:.2e}, pad columns {pad:.2e}")
    assert eig <= 1e-11, (tag, eig)
    assert np.all(np.diff(wk) >= 0), f"{tag}: eigenvalues not ascending"
    assert res <= 1e-10, (tag, res)
    assert orth <= 1e-10, (tag, orth)
    assert pad <= 1e-13, (tag, pad)


def _check_index_solve(tag, s, mats, lo, hi):
    per = s.results()
    v_all = s.v.cpu().numpy()
    assert tuple(s.w.shape) == (len(mats), hi - lo + 1) and v_all.shape == (len(mats), hi - lo + 1, s.order)
    for b, mat in enumerate(mats):
        own = len(mat)
        wk, vk = per[b][0].cpu().numpy(), per[b][1].cpu().numpy()
        pad = np.abs(v_all[b, :, own:]).max() if own < s.order else 0.0
        _check_rows(f"{tag} [{lo}, {hi}] structure {b}", mat, np.linalg.eigvalsh(mat), np.arange(lo, hi + 1), wk, vk, pad,
                    _slot_scale(mat))


# ---- 4. index range, one-stage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 11), (6, 25)])
def test_index_range_mixed_force_fields_one_stage(torch, mixed, lo, hi):
    s = _solver(mixed["sizes"], mixed["ffs"], masses=mixed["masses"], order=192, subset_by_index=(lo, hi))
    assert s.order == 192
    s.set_profiling(True)
    s.solve(_packed(torch, mixed["coords"]))
    s.finish()
    if forced_two_stage() is None:
        assert not s.last_timings()["two_stage"]
    _check_index_solve("one-stage", s, mixed["mats"], lo, hi)


# ---- 5. index range, two-stage forced -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(86, 100, 70, 93), (86, 101, 70)])
def test_index_range_two_stage(sc, torch, sizes):
    coords = [synthetic_coord(n, 320 + k) for k, n in enumerate(sizes)]
    mats = [orc.compute_hessian(c, orc.invariant_ff(13.0))[0] for c in coords]
    s = _solver(sizes, sc.InvariantForceField(13.0), subset_by_index=(0, 25))
    assert s.order == 3 * max(sizes)
    s.ctx.set_two_stage(True)
    s.set_profiling(True)
    s.solve(_packed(torch, coords))
    s.finish()
    if forced_two_stage() is not False:
        assert s.last_timings()["two_stage"]
    _check_index_solve(f"two-stage order {s.order}", s, mats, 0, 25)


# ---- 6. index range, GNM ------------------------------------------------------------------------------------------------------
def test_index_range_gnm(sc, torch):
    sizes = (150, 171, 200)
    coords = [synthetic_coord(n, 330 + k) for k, n in enumerate(sizes)]
    mats = [orc.compute_kirchhoff(c, orc.invariant_ff(10.0))[0] for c in coords]
    s = _solver(sizes, sc.InvariantForceField(10.0), dim=1, subset_by_index=(0, 9))
    s.solve(_packed(torch, coords))
    s.finish()
    _check_index_solve("gnm", s, mats, 0, 9)


def test_index_range_is_checked_against_the_smallest_structure(sc):
    with pytest.raises(ValueError, match=r"smallest structure \(2: 37 atoms\)"):
        _solver(MIXED_SIZES, sc.InvariantForceField(13.0), subset_by_index=(0, 111))


# ---- 7. window ------------------------------------------------------------------------------------------------------------------
def _gap_above_trivial(mixed):
    """Midpoint of the gap above the six trivial modes of the stiffest structure (largest slot norm)."""
    stiff = int(np.argmax([_slot_scale(m) for m in mixed["mats"]]))
    w = mixed["spectra"][stiff]
    return 0.5 * (w[5] + w[6])


def _window_bounds(mixed):
    """
    (vl, vu): vl the midpoint of the gap above the trivial modes of the stiffest structure, vu the midpoint of the widest gap of the pooled reference spectra
    among the 40 gaps around the median 45th eigenvalue.  Asserts that no reference eigenvalue of a structure lies within
    1e-8 S of a bound, so the counts are decided.
    """
    vl = _gap_above_trivial(mixed)
    pooled = np.sort(np.concatenate(mixed["spectra"]))
    at = int(np.searchsorted(pooled, np.median([w[45] for w in mixed["spectra"]])))
    cand = np.arange(max(at - 20, 1), min(at + 20, len(pooled) - 1))
    i = cand[np.argmax(pooled[cand + 1] - pooled[cand])]
    vu = 0.5 * (pooled[i] + pooled[i + 1])
    for w, mat in zip(mixed["spectra"], mixed["mats"]):
        for bound in (vl, vu):
            assert np.abs(w - bound).min() > 1e-8 * _slot_scale(mat)
        assert np.abs(w[:6]).max() < vl      # (softer structures may have modes below vl: il differs per structure)
    return vl, vu


def _check_window_slots(tag, s, mixed, vl, vu, K):
    counts = s.counts.cpu().numpy()
    w_all, v_all = s.w.cpu().numpy(), s.v.cpu().numpy()
    per = s.results()
    for b, (mat, w_ref) in enumerate(zip(mixed["mats"], mixed["spectra"])):
        own = len(mat)
        il = int(np.sum(w_ref <= vl))
        cnt = int(np.sum(w_ref <= vu)) - il
        assert counts[b] == cnt, (tag, b, counts[b], cnt)
        keep = min(cnt, K)
        assert np.all(np.isnan(w_all[b, keep:])) and not np.any(v_all[b, keep:]), (tag, b)
        wk, vk = per[b][0].cpu().numpy(), per[b][1].cpu().numpy()
        pad = np.abs(v_all[b, :, own:]).max() if own < s.order else 0.0
        _check_rows(f"{tag} structure {b} ({cnt} in the window)", mat, w_ref, np.arange(il, il + keep), wk, vk, pad,
                    _slot_scale(mat))


def test_window_counts_and_slots(torch, mixed):
    vl, vu = _window_bounds(mixed)
    K = 3 * min(mixed["sizes"])
    s = _solver(mixed["sizes"], mixed["ffs"], masses=mixed["masses"], subset_by_value=(vl, vu), max_modes=K)
    assert tuple(s.w.shape) == (4, K) and tuple(s.v.shape) == (4, K, 192)
    s.solve(_packed(torch, mixed["coords"]))
    assert s.counts.dtype == torch.int64 and s.counts.is_cuda
    s.finish()
    _check_window_slots("window", s, mixed, vl, vu, K)


def test_window_to_infinity_never_counts_the_pads_and_overflow_is_named(sc, torch):
    """
    (vl, +inf) on sizes (20, 64) with K = 60: the small structure's slot holds 132 pad eigenvalues above its own 60; its
    count is 60 - il exactly and its rows are its own top modes.  The large one holds 192 - il > K eigenpairs: finish() names it.
    """
    sizes = (20, 64)
    coords = [synthetic_coord(n, 340 + k) for k, n in enumerate(sizes)]
    mats = [orc.compute_hessian(c, orc.invariant_ff(13.0))[0] for c in coords]
    spectra = [np.linalg.eigvalsh(h) for h in mats]
    data = dict(mats=mats, spectra=spectra)
    vl = _gap_above_trivial(data)
    for w, mat in zip(spectra, mats):
        assert np.abs(w - vl).min() > 1e-8 * _slot_scale(mat) and np.abs(w[:6]).max() < vl
    expect = [3 * n - int(np.sum(w <= vl)) for n, w in zip(sizes, spectra)]
    assert expect[0] <= 54 and expect[1] > 60
    K = 60
    s = _solver(sizes, sc.InvariantForceField(13.0), subset_by_value=(vl, np.inf), max_modes=K)
    s.solve(_packed(torch, coords))
    with pytest.raises(ValueError, match=rf"structure\(s\) 1 \({expect[1]}\)"):
        s.finish()
    counts = s.counts.cpu().numpy()
    print(f"counts {counts.tolist()} for own orders {[3 * n for n in sizes]} in slots of {s.order}")
    assert counts.tolist() == expect
    _check_window_slots("(vl, inf)", s, data, vl, np.inf, K)
    # and a window wholly above the structure's spectrum but inside the pads' range: nothing
    top = max(w[-1] for w in spectra)
    s = _solver(sizes, sc.InvariantForceField(13.0), subset_by_value=(1.001 * top, np.inf), max_modes=K)
    s.solve(_packed(torch, coords))
    s.finish()
    assert s.counts.cpu().numpy().tolist() == [0, 0]
    assert np.all(np.isnan(s.w.cpu().numpy())) and not np.any(s.v.cpu().numpy())


# ---- 8. consumers, full spectrum, tile boundaries --------------------------------------------------------------------------------
def _lapack_dcc(mat, n, dim):
    cov = np.linalg.pinv(mat, hermitian=True, rcond=1e-6)
    return cov.reshape(n, dim, n, dim).swapaxes(1, 2).trace(axis1=2, axis2=3)


@pytest.mark.parametrize("sizes", [(150, 171, 200, 183), (150, 171, 201)])
def test_consumers_full_spectrum_across_the_column_tiles(sc, torch, sizes):
    """
    Order 600: own orders 450 (the second 512-column tile is all pad), 513 (one own column in it), 600 (no pad), 549;
    order 603 is odd, the 8-byte form of the msf loads.
    """
    dim, ntriv = 3, 6
    coords = [synthetic_coord(n, 350 + k) for k, n in enumerate(sizes)]
    mats = [orc.compute_hessian(c, orc.invariant_ff(13.0))[0] for c in coords]
    s = _solver(sizes, sc.InvariantForceField(13.0))
    assert s.order == 3 * max(sizes)
    s.solve(_packed(torch, coords))
    s.finish()
    pairs = [(w.cpu().numpy(), v.cpu().numpy()) for w, v in s.results()]
    listed = np.array([7, 30, 449, 7, 12])
    for name, subset in (("default", None), ("list with a repeat", listed)):
        msf = s.mean_square_fluctuation(mode_subset=subset)
        bfac = s.bfactor(mode_subset=subset)
        raw = s.dcc(mode_subset=subset, norm=False)
        nrm = s.dcc(mode_subset=subset)
        tem = s.dcc(mode_subset=subset, tem=300, tem_factors=K_B * N_A)
        mtem = s.mean_square_fluctuation(mode_subset=subset, tem=300, tem_factors=K_B * N_A)
        for b, n in enumerate(sizes):
            tag = f"order {s.order} structure {b} (own {dim * n}) {name}"
            w, v = pairs[b]
            assert msf[b].is_cuda and tuple(msf[b].shape) == (n,) and tuple(raw[b].shape) == (n, n), tag
            assert tuple(nrm[b].shape) == (n, n) and tuple(bfac[b].shape) == (n,)
            rows = np.arange(ntriv, dim * n) if subset is None else subset
            got = msf[b].cpu().numpy()
            check_msf(got, np_msf(w, v, rows, dim), rows, dim, tag)
            assert np.array_equal(bfac[b].cpu().numpy(), got * ((8 * np.pi**2) / 3))
            assert np.array_equal(mtem[b].cpu().numpy(), got * (300 * (K_B * N_A)))
            drows = pinv_rows(w) if subset is None else rows
            ref = np_dcc(w, v, drows, dim)
            check_dcc(raw[b].cpu().numpy(), ref, drows, dim, tag)
            check_dcc_norm(nrm[b].cpu().numpy(), ref, drows, dim, tag)
            assert np.array_equal(tem[b].cpu().numpy(), nrm[b].cpu().numpy() * 300 * (K_B * N_A))
            if subset is None:      # the meaning: LAPACK on the oracle's matrix
                wl, vl = np.linalg.eigh(mats[b])
                mref = np_msf(wl, vl.T, rows, dim)
                assert np.allclose(got, mref, rtol=1e-8, atol=1e-9 * np.abs(mref).max()), tag
                tr = _lapack_dcc(mats[b], n, dim)
                d = np.sqrt(np.diag(tr))
                assert np.allclose(raw[b].cpu().numpy(), tr, rtol=1e-8, atol=1e-9 * np.abs(tr).max()), tag
                assert np.allclose(nrm[b].cpu().numpy(), tr / np.outer(d, d), rtol=1e-8, atol=1e-9), tag
    # a mode the smallest structure does not have is refused for the whole batch
    with pytest.raises(ValueError, match="mode 450 was not solved"):
        s.mean_square_fluctuation(mode_subset=[7, 450])
    with pytest.raises(ValueError, match="Trivial modes"):
        s.dcc(mode_subset=[5, 7])


# ---- 9. the pinv default per structure ----------------------------------------------------------------------------------------------
def test_dcc_default_takes_the_pinv_maximum_over_the_structures_own_spectrum(sc, torch):
    """
    GNM (30, 64), Invariant 7 A.  The 30-atom structure is two clusters joined by one spring of 4e-4: its second
    eigenvalue is 3.6e-6 of its own largest one, but 4.8e-7 of the slot's largest pad value.  The rule keeps it; a
    threshold taken over the whole slot would drop it.
    """
    rs = np.random.RandomState(11)
    two = np.concatenate([rs.rand(15, 3) * 6.0, rs.rand(15, 3) * 6.0 + np.array([40.0, 0.0, 0.0])])
    coords = [two, synthetic_coord(64, 360)]
    link = dict(contact_pair_on=np.array([[0, 15]]), force_constants=np.array([4e-4]))
    ffs = [sc.PatchedForceField(sc.InvariantForceField(7.0), **link), sc.InvariantForceField(7.0)]
    mats = [orc.compute_kirchhoff(two, oracle_patched(orc.invariant_ff(7.0), 30, **link))[0],
            orc.compute_kirchhoff(coords[1], orc.invariant_ff(7.0))[0]]
    s = _solver((30, 64), ffs, dim=1)
    s.solve(_packed(torch, coords))
    raw, nrm = s.dcc(norm=False), s.dcc()
    s.finish()
    slot_w = s.w.cpu().numpy()
    changed = 0
    for b in range(2):
        w, v = (x.cpu().numpy() for x in s.results()[b])
        own_rows = pinv_rows(w)
        slot_rows = np.nonzero(np.abs(w) > 1e-6 * np.abs(slot_w[b]).max())[0]
        changed += len(own_rows) != len(slot_rows)
        print(f"structure {b}: {len(own_rows)} modes by its own maximum {np.abs(w).max():.3e}, {len(slot_rows)} by the "
              f"slot's {np.abs(slot_w[b]).max():.3e}")
        ref = np_dcc(w, v, own_rows, 1)
        check_dcc(raw[b].cpu().numpy(), ref, own_rows, 1, f"pinv rule [{b}]")
        check_dcc_norm(nrm[b].cpu().numpy(), ref, own_rows, 1, f"pinv rule [{b}]")
    assert len(pinv_rows(s.results()[0][0].cpu().numpy())) == 29
    assert changed >= 1      # otherwise this case proves nothing


# ---- 10. consumers behind an index range and behind a window ------------------------------------------------------------------------
def test_consumers_behind_an_index_range(torch, mixed):
    dim, ntriv = 3, 6
    for lo, hi in ((0, 11), (6, 25)):
        s = _solver(mixed["sizes"], mixed["ffs"], masses=mixed["masses"], subset_by_index=(lo, hi))
        s.solve(_packed(torch, mixed["coords"]))
        msf, raw, nrm = s.mean_square_fluctuation(), s.dcc(norm=False), s.dcc()
        sub = s.mean_square_fluctuation(mode_subset=[hi, max(lo, ntriv), hi])
        freq = s.frequencies()
        s.finish()
        for b, n in enumerate(mixed["sizes"]):
            w, v = (x.cpu().numpy() for x in s.results()[b])
            rows = np.arange(max(ntriv - lo, 0), hi - lo + 1)          # every solved non-trivial row
            tag = f"index [{lo}, {hi}] structure {b}"
            check_msf(msf[b].cpu().numpy(), np_msf(w, v, rows, dim), rows, dim, tag)
            ref = np_dcc(w, v, rows, dim)
            check_dcc(raw[b].cpu().numpy(), ref, rows, dim, tag)
            check_dcc_norm(nrm[b].cpu().numpy(), ref, rows, dim, tag)
            lrows = np.array([hi - lo, max(lo, ntriv) - lo, hi - lo])
            check_msf(sub[b].cpu().numpy(), np_msf(w, v, lrows, dim), lrows, dim, tag + " list")
            k = max(ntriv - lo, 0)
            fref = np.sqrt(np.concatenate([np.abs(w[:k]), w[k:]])) / (2 * np.pi)
            assert tuple(freq[b].shape) == (hi - lo + 1,) and np.allclose(freq[b].cpu().numpy(), fref, rtol=1e-14)


def test_consumers_behind_a_window_and_an_empty_window(torch, mixed):
    dim = 3
    vl, vu = _window_bounds(mixed)
    K = 3 * min(mixed["sizes"])
    s = _solver(mixed["sizes"], mixed["ffs"], masses=mixed["masses"], subset_by_value=(vl, vu), max_modes=K)
    s.solve(_packed(torch, mixed["coords"]))
    msf, raw, nrm = s.mean_square_fluctuation(), s.dcc(norm=False), s.dcc()
    s.finish()
    counts = s.counts.cpu().numpy()
    for b, n in enumerate(mixed["sizes"]):
        w, v = (x.cpu().numpy() for x in s.results()[b])
        rows = np.arange(min(counts[b], K))
        assert len(w) == len(rows) > 0
        tag = f"window structure {b} ({len(rows)} rows)"
        check_msf(msf[b].cpu().numpy(), np_msf(w, v, rows, dim), rows, dim, tag)
        ref = np_dcc(w, v, rows, dim)
        check_dcc(raw[b].cpu().numpy(), ref, rows, dim, tag)
        check_dcc_norm(nrm[b].cpu().numpy(), ref, rows, dim, tag)
    with pytest.raises(ValueError, match="cannot be combined"):
        s.mean_square_fluctuation(mode_subset=[7])
    # an empty window: between the trivial modes and the softest structure's first mode
    first = min(w[6] for w in mixed["spectra"])
    assert max(np.abs(w[:6]).max() for w in mixed["spectra"]) < 1e-6 * first
    s = _solver(mixed["sizes"], mixed["ffs"], masses=mixed["masses"], subset_by_value=(0.25 * first, 0.5 * first),
                max_modes=K)
    s.solve(_packed(torch, mixed["coords"]))
    msf, raw, nrm = s.mean_square_fluctuation(), s.dcc(norm=False), s.dcc()
    s.finish()
    assert s.counts.cpu().numpy().tolist() == [0, 0, 0, 0]
    for b, n in enumerate(mixed["sizes"]):
        assert tuple(msf[b].shape) == (n,) and not np.any(msf[b].cpu().numpy())
        assert not np.any(raw[b].cpu().numpy()) and np.all(np.isnan(nrm[b].cpu().numpy()))
        assert tuple(s.results()[b][0].shape) == (0,)


# ---- 11. placement independence ---------------------------------------------------------------------------------------------------------
def test_a_structures_bits_do_not_depend_on_its_slot(sc, torch):
    dim = 3
    sizes = (150, 200, 150)
    x = synthetic_coord(150, 370)
    coords = [x, synthetic_coord(200, 371), x]
    s = _solver(sizes, sc.InvariantForceField(13.0))
    s.solve(_packed(torch, coords))
    s.finish()
    s.w[2].copy_(s.w[0]); s.v[2].copy_(s.v[0])
    w, v = (t.cpu().numpy() for t in s.results()[0])
    rows = pinv_rows(w)
    ref = np_dcc(w, v, rows, dim)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    tol = 4 * len(rows) * dim * EPS
    for subset in (None, np.arange(6, 36)):
        m = [t.cpu().numpy() for t in s.mean_square_fluctuation(mode_subset=subset)]
        assert np.array_equal(m[0], m[2])
    free = {}
    for norm in (False, True):
        d = [t.cpu().numpy() for t in s.dcc(norm=norm)]
        assert np.array_equal(d[0], d[2])
        free[norm] = d
    # 64 KiB hold 6 rows of order 600 in both packed operands: every structure a slab of its own, 100 row chunks
    from springcraft_amd import _hip

    L = _hip.lib()
    assert L.sc_batch_plan_modes_workspace_bytes(s._plan, 600, 600, 1, 64 << 10) < \
        L.sc_batch_plan_modes_workspace_bytes(s._plan, 600, 600, 1, 0)
    s.consumer_budget_bytes = 64 << 10
    for norm in (False, True):
        d = [t.cpu().numpy() for t in s.dcc(norm=norm)]
        assert np.array_equal(d[0], d[2])
        (check_dcc_norm if norm else check_dcc)(d[0], ref, rows, dim, f"64 KiB budget norm={norm}")
        if not norm:
            err = np.abs(d[0] - free[norm][0])
            print(f"small budget against the unconstrained call: {(err / scale).max():.3e}, bound {2 * tol:.3e}")
            assert np.all(err <= 2 * tol * scale)
        else:
            assert np.abs(d[0] - free[norm][0]).max() <= 2 * 3 * tol
        assert np.array_equal(d[1].shape, (200, 200))
    s.consumer_budget_bytes = None


# ---- 12. a failed structure -----------------------------------------------------------------------------------------------------------------
def test_a_nan_structure_gives_nan_and_leaves_its_neighbours_their_bits(sc, torch):
    sizes = (40, 50, 45)
    coords = [synthetic_coord(n, 380 + k) for k, n in enumerate(sizes)]
    ff = sc.HinsenForceField()                      # no cutoff: a NaN coordinate reaches the matrix
    good = _solver(sizes, ff)
    good.solve(_packed(torch, coords))
    good.finish()
    ref = [good.mean_square_fluctuation(), good.dcc(), good.dcc(mode_subset=np.arange(6, 36), norm=False)]
    broken = [c.copy() for c in coords]
    broken[1][7, 2] = np.nan
    bad = _solver(sizes, ff)
    bad.solve(_packed(torch, broken))
    got = [bad.mean_square_fluctuation(), bad.dcc(), bad.dcc(mode_subset=np.arange(6, 36), norm=False)]
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    assert np.all(np.isnan(bad.w.cpu().numpy()[1]))
    for g, r in zip(got, ref):
        assert np.all(np.isnan(g[1].cpu().numpy()))
        for b in (0, 2):
            assert np.array_equal(g[b].cpu().numpy(), r[b].cpu().numpy())


# ---- 13. the reference's fixtures ---------------------------------------------------------------------------------------------------------------
def test_1l2y_in_a_ragged_batch_reproduces_the_prody_fixtures(sc, torch):
    ca = structures()["1l2y_coord"]
    assert len(ca) == 20
    coords = [np.asarray(ca, dtype=np.float64), synthetic_coord(50, 390)]
    s = _solver((20, 50), sc.InvariantForceField(13))
    s.solve(_packed(torch, coords))
    msf, dcc, freq = s.mean_square_fluctuation(), s.dcc(), s.frequencies()
    s.finish()
    name = "prody_anm_13_ang_cutoff"
    assert np.allclose(msf[0].cpu().numpy(), load_csv(f"{name}_fluctuations_1l2y.csv.gz"))
    assert np.allclose(dcc[0].cpu().numpy(), load_csv(f"{name}_dcc_norm_1l2y.csv.gz"))
    evals = load_csv(f"{name}_evals_1l2y.csv.gz")
    assert tuple(freq[0].shape) == (60,) and np.allclose(freq[0].cpu().numpy()[6:], np.sqrt(evals[6:]) / (2 * np.pi))
    anm = sc.ANM(coords[1], sc.InvariantForceField(13))
    assert np.allclose(msf[1].cpu().numpy(), anm.mean_square_fluctuation())
    assert np.allclose(dcc[1].cpu().numpy(), anm.dcc())


# ---- 14. nothing synchronises ---------------------------------------------------------------------------------------------------------------------
def test_consumers_enqueued_straight_behind_solve_give_the_same_bits(sc, torch):
    sizes = (150, 171, 201)
    coords = _packed(torch, [synthetic_coord(n, 400 + k) for k, n in enumerate(sizes)])
    ff = sc.InvariantForceField(13.0)

    def consumers(s):
        out = s.mean_square_fluctuation() + s.dcc() + s.dcc(mode_subset=[9, 7, 9], norm=False) + s.bfactor() + s.frequencies()
        return out

    a = _solver(sizes, ff)
    a.solve(coords)
    a.finish()
    torch.cuda.synchronize()
    ref = consumers(a)
    torch.cuda.synchronize()
    b = _solver(sizes, ff)
    consumers(b)                  # (workspaces allocated: the calls below only enqueue)
    torch.cuda.synchronize()
    b.solve(coords)
    got = consumers(b)
    torch.cuda.synchronize()
    b.finish()
    assert len(got) == len(ref) == 15
    for g, r in zip(got, ref):
        assert np.array_equal(g.cpu().numpy(), r.cpu().numpy())
