"""
Stage-level backward-error tests of the eigensolver: the reconstruction and orthogonality ratios of LAPACK's test programs
(tests/stage_ratios.py), in units of n ulp, for every stage on every kernel form the product can take -- the band
reduction (A = Q1 B Q1^T), the bulge chase with the diamond back-transformation (B = Q2 T Q2^T), both together
(A = Q T Q^T), the one-stage reductions, and the tridiagonal divide & conquer (T = Z diag(w) Z^T) -- through the staged
debug entries sc_dbg_reduce_host / sc_dbg_stedc_host, which launch the product's kernels through the product's host
functions.  Private contexts; path and form forced as in tests/test_two_stage_gpu.py and
tests/test_batched_degenerate_gpu.py and confirmed by the same counters; every member of every batch is checked; the
figures are printed before anything is asserted.  Every ratio is gated at 50, a thousand to ten thousand times tighter than
the end-to-end max-abs gates at these orders; LAPACK's own factors stay below 5 on the same inputs
(tests/test_stage_ratios_host.py).  profiles/stage_ratios.txt holds the figures of the first run.

The test_form_* cases at the end hold one kernel form each to the same gate, at the smallest shape at which the policy
(csrc/twostage_policy.h) selects it, and prove by the context's form counters that it ran: the expected counts are the
literals of tests/host_sanitize/test_host_logic.cpp, derived by hand from the rules.  Not covered there:
k_bt2_apply<8> on the (chunk, matrix) grid (it needs n >= 4609 at batch 7, and there is no in-process override), the
partial-spectrum Q2 (ncols < n: tests/test_partial_ratios_gpu.py), and stedc above n = 2048 (n > 7000:
tests/test_large_order_gpu.py).
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests import stage_ratios as sr

pytestmark = pytest.mark.gpu

CHASE_COUNTERS = ("chase_launches", "chase_timeouts", "chase_incomplete", "chase_resumed", "chase_sweeps", "stepwise_chases",
                  "chase_pair_launches", "chase_pair_fallbacks")


@pytest.fixture()
def lib_ctx():
    from springcraft_amd import _hip

    L = sr.debug_lib()
    ctx = _hip.Context(0)
    try:
        yield L, ctx
    finally:
        ctx.close()


def batch_of(kind, n):
    """(member names, batch) -- a batch of one random matrix, or the mixed batch."""
    if kind == "one":
        return ["random"], sr.random_sym(n)[None]
    return sr.mixed_batch(n)


def scaled(a, s):
    """s A with s the power of two the solver scaled the matrix by (exact)."""
    assert s > 0.0 and np.frexp(s)[0] == 0.5, s
    return a * s


def report(label, rows):
    """rows: (member, {figure: value}); prints all of them, then asserts every one against the gate."""
    failures = []
    for name, figures in rows:
        print(f"[{label}] {name:<10s} " + "  ".join(f"{k} {v:.3g}" for k, v in figures.items()))
        for k, v in figures.items():
            if k == "beyond_band":
                if v != 0.0:
                    failures.append((name, k, v))
            elif not v <= sr.GATE:
                failures.append((name, k, v))
    assert not failures, (label, failures)


def check_two_stage(L, ctx, label, names, mats, counters):
    """The three factors of the two-stage path; `counters(call)` confirms the forced form after each call."""
    n = mats.shape[1]
    out = {}
    for which in (sr.Q_ONE, sr.Q_TWO, sr.Q_ALL):
        out[which] = sr.reduce_host(L, ctx, mats, which)
        assert out[which][5], "the two-stage path was forced"
        counters(len(out))
    rows = []
    for b, name in enumerate(names):
        fig = {}
        d, e, s, band, q1, _ = (x[b] if isinstance(x, np.ndarray) else x for x in out[sr.Q_ONE])
        a = scaled(mats[b], s)
        fig["recon(A,Q1,B)"] = sr.recon(a, q1, sr.band_matrix(band))
        fig["orth(Q1)"] = sr.orth(q1)
        fig["beyond_band"] = sr.band_beyond(band)
        d, e, s, band, q2, _ = (x[b] if isinstance(x, np.ndarray) else x for x in out[sr.Q_TWO])
        fig["recon(B,Q2,T)"] = sr.recon(sr.band_matrix(band), q2, sr.tridiagonal(d, e))
        fig["orth(Q2)"] = sr.orth(q2)
        fig["beyond_band"] = max(fig["beyond_band"], sr.band_beyond(band))
        d, e, s, band, q, _ = (x[b] if isinstance(x, np.ndarray) else x for x in out[sr.Q_ALL])
        fig["recon(A,Q,T)"] = sr.recon(scaled(mats[b], s), q, sr.tridiagonal(d, e))
        fig["orth(Q)"] = sr.orth(q)
        rows.append((name, fig))
    report(label, rows)
    return out


def check_one_stage(L, ctx, label, names, mats):
    d, e, s, band, q, two = sr.reduce_host(L, ctx, mats, sr.Q_ALL)
    assert not two and band is None
    rows = []
    for b, name in enumerate(names):
        rows.append((name, {"recon(A,Q,T)": sr.recon(scaled(mats[b], s[b]), q[b], sr.tridiagonal(d[b], e[b])),
                            "orth(Q)": sr.orth(q[b])}))
    report(label, rows)
    return d, e, s, q


def chase_check(ctx, form, give_up, n, batch):
    def check(calls):
        cnt = {k: ctx.counter(k) for k in CHASE_COUNTERS}
        assert cnt["chase_launches"] == calls and cnt["stepwise_chases"] == 0, cnt
        assert cnt["chase_pair_launches"] == (calls if form == 3 else 0) and cnt["chase_pair_fallbacks"] == 0, cnt
        assert cnt["chase_timeouts"] == 0 and cnt["chase_incomplete"] == 0, cnt
        if give_up == 0:
            assert cnt["chase_resumed"] == 0 and cnt["chase_sweeps"] == calls * batch * (n - 2), cnt
        else:
            assert cnt["chase_resumed"] == calls and cnt["chase_sweeps"] < calls * batch * (n - 2), cnt
    return check


# ---- two-stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind,give_up", [(256, "one", 0), (322, "one", 0), (322, "mixed", 0), (322, "one", 5),
                                            (322, "mixed", 5), (1030, "one", 5)])
@pytest.mark.parametrize("form", [3, 4, 5])
def test_two_stage_chase_forms(lib_ctx, form, n, kind, give_up):
    """
    The persistent chase in the pair form (3), with one sweep per workgroup (4) and spread over all XCDs (5; the mixed
    batch has seven members, fewer than the device has XCDs), stage 1 by the default panel kernels.  n = 256: the minimum;
    322: partial last panel, diamond and sweep group; give_up = 5: every workgroup gives up after five tasks and
    k_chase_finish takes over -- at n = 1030 with sixteen sweep groups behind it.
    """
    L, ctx = lib_ctx
    names, mats = batch_of(kind, n)
    ctx.set_two_stage(True)
    ctx.check(L.sc_dbg_set_chase(ctx.handle, form, give_up))
    check_two_stage(L, ctx, f"two-stage n={n} {kind} form={form} give_up={give_up}", names, mats,
                    chase_check(ctx, form, give_up, n, len(names)))


def coop_overridden():
    return os.environ.get("SPRINGCRAFT_QR_COOP") == "0" or bool(os.environ.get("SPRINGCRAFT_QR_COOP_MIN")) or \
        int(os.environ.get("SPRINGCRAFT_STAGE1_STREAMS") or 0) > 1


@pytest.mark.parametrize("n,kind,min_rows,fail_panel", [(322, "one", 0, -1), (322, "mixed", 0, -1),
                                                        (322, "one", 128, -1), (322, "mixed", 128, -1),
                                                        (322, "one", 128, 1), (322, "mixed", 128, 1),
                                                        (1030, "one", 200, -1), (1030, "one", 200, 2)])
def test_two_stage_panel_kernels(lib_ctx, n, kind, min_rows, fail_panel):
    """
    Stage 1 by the single-workgroup panel kernels alone (k_panel_wg: min_rows 0 keeps k_panel_coop out), by k_panel_coop
    (panels of at least min_rows rows: two workgroups per matrix at n = 322, four at n = 1030), and with its take-over
    k_panel_serial from panel `fail_panel` on.
    """
    if min_rows and coop_overridden():
        pytest.skip("the cooperative kernel's rule is overridden (tools/test_matrix.sh)")
    L, ctx = lib_ctx
    names, mats = batch_of(kind, n)
    batch = len(names)
    ctx.set_two_stage(True)
    ctx.check(L.sc_dbg_set_panel_coop(ctx.handle, min_rows))
    ctx.check(L.sc_dbg_set_panel_coop_fail(ctx.handle, fail_panel))
    coop_panels = sum(1 for p in range(n // 64 + 1) if n - (p + 1) * 64 >= max(min_rows, 65)) if min_rows else 0

    def counters(calls):
        launches, timeouts = ctx.counter("panel_coop_launches"), ctx.counter("panel_coop_timeouts")
        if fail_panel < 0:
            assert launches == calls * coop_panels and timeouts == 0, (launches, timeouts)
        else:
            # the first call meets the hook, counts every panel behind it, and the context then keeps to the chunked
            # launches until the hook is set again (below)
            assert coop_panels > fail_panel
            assert launches == calls * coop_panels and timeouts == calls * batch * (coop_panels - fail_panel), \
                (launches, timeouts)
            ctx.check(L.sc_dbg_set_panel_coop_fail(ctx.handle, fail_panel))
        assert ctx.counter("chase_timeouts") == 0 and ctx.counter("chase_incomplete") == 0

    check_two_stage(L, ctx, f"two-stage n={n} {kind} coop_min_rows={min_rows} fail_panel={fail_panel}", names, mats, counters)


def test_two_stage_minimum_order(lib_ctx):
    L, ctx = lib_ctx
    ctx.set_two_stage(True)
    rc, _ = sr.reduce_raw(L, ctx, sr.random_sym(130)[None], sr.Q_ALL)
    assert rc == 1, rc          # SC_ERR_INVALID_ARG
    ctx.set_two_stage(False)
    rc, _ = sr.reduce_raw(L, ctx, sr.random_sym(130)[None], sr.Q_TWO)
    assert rc == 1, rc          # the one-stage path has one factor


# ---- one-stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 322])
def test_one_stage_batched(lib_ctx, n):
    """The batched launch-per-column tridiagonalisation and the Q1 back-transformation with off = 1, on the mixed batch."""
    L, ctx = lib_ctx
    names, mats = sr.mixed_batch(n)
    ctx.set_two_stage(False)
    check_one_stage(L, ctx, f"one-stage n={n} mixed", names, mats)
    assert ctx.counter("chase_launches") == 0 and ctx.counter("stepwise_chases") == 0
    assert ctx.counter("resident_launches") == 0


@pytest.mark.parametrize("n,hook", [(322, 0), (2050, 0), (322, 1), (322, 2 + 150)])
def test_one_stage_resident(lib_ctx, n, hook):
    """k_sytrd_resident on one matrix: the rows in LDS (n = 322) and in registers (n = 2050), and k_sytrd_takeover behind
    a failed roll call (hook 1) and behind a wait lost at step 150 (hook 2 + 150)."""
    if os.environ.get("SPRINGCRAFT_RESIDENT") == "0" or n > int(os.environ.get("SPRINGCRAFT_RESIDENT_MAX", "3072")):
        pytest.skip("the kernel under test is switched off or limited (tools/test_matrix.sh)")
    L, ctx = lib_ctx
    ctx.set_two_stage(False)
    ctx.check(L.sc_dbg_set_resident(ctx.handle, 1, hook, 0))
    check_one_stage(L, ctx, f"one-stage resident n={n} hook={hook}", ["random"], sr.random_sym(n)[None])
    assert ctx.counter("resident_launches") == 1
    assert ctx.counter("resident_takeovers") == (1 if hook else 0)
    print({k: ctx.counter(k) for k in ("resident_rollcall_failures", "resident_lost_waits")})


# ---- tridiagonal solver ---------------------------------------------------------------------------------------------------
def stedc_orders(L):
    leaf = L.sc_dbg_stedc_leaf_max(1000)
    return [2, leaf, leaf + 1, 322, 1000]


@pytest.mark.parametrize("slot", range(5))
def test_tridiagonal_solver(lib_ctx, slot):
    """
    stedc_batched alone, one batch per order with all the inputs together: n = 2, the largest leaf (QL only), one more (the
    smallest merge), 322 and 1000.  T = Z diag(w) Z^T and Z orthogonal to the gate; by Weyl's theorem these two bound the
    eigenvalue errors as well, so only the (1, 2, 1) Toeplitz matrix, whose spectrum is known exactly, has a gate on them.
    """
    L, ctx = lib_ctx
    n = stedc_orders(L)[slot]
    assert L.sc_dbg_stedc_leaf_max(n) == 32, "tests/test_stage_ratios_host.py checks LAPACK at orders 32 and 33"
    inputs = sr.tridiagonal_inputs(n)
    d = np.stack([inputs[k][0] for k in sr.TRIDIAGONALS])
    e = np.stack([inputs[k][1] for k in sr.TRIDIAGONALS])
    w, z = sr.stedc_host(L, ctx, d, e)
    rows = []
    for b, name in enumerate(sr.TRIDIAGONALS):
        fig = {"recon(T,Z,w)": sr.recon(sr.tridiagonal(d[b], e[b]), z[b], np.diag(w[b])), "orth(Z)": sr.orth(z[b])}
        if name == "toeplitz":
            fig["eig/(4 n ulp)"] = np.abs(w[b] - sr.toeplitz_exact(n)).max() / (4 * n * sr.ULP)
        assert np.all(np.diff(w[b]) >= 0.0), (name, "eigenvalues not ascending")
        rows.append((name, fig))
    report(f"stedc n={n}", rows)


def test_tridiagonal_solver_is_independent_of_the_batch_slot(lib_ctx):
    """Eight copies of one input in one batch: every Z and w is bit-identical, and passes the gate."""
    L, ctx = lib_ctx
    n = 322
    d0, e0 = sr.tridiagonal_inputs(n)["glued1e-4"]
    w, z = sr.stedc_host(L, ctx, np.tile(d0, (8, 1)), np.tile(e0, (8, 1)))
    report(f"stedc n={n} x 8", [("glued1e-4", {"recon(T,Z,w)": sr.recon(sr.tridiagonal(d0, e0), z[0], np.diag(w[0])),
                                               "orth(Z)": sr.orth(z[0])})])
    for b in range(1, 8):
        assert np.array_equal(w[b], w[0]) and np.array_equal(z[b], z[0]), b


@pytest.mark.parametrize("n", [255, 256, 1023, 1024, 2047, 2048])
def test_tridiagonal_solver_at_the_launch_thresholds(lib_ctx, n):
    """
    stedc_batched at the orders on both sides of every step of its thread and LDS table (csrc/stedc_plan.h:dc_level_launch:
    the top merge has n rows; k_dc_setup 64 / 256 / 1024 threads from 256 and 1024 rows, k_dc_secular 256 / 1024 from 2048),
    a batch of two different matrices: a random tridiagonal matrix and the glued Wilkinson blocks.  The ratios and the gate
    of test_tridiagonal_solver, formed on the device (sr.recon_t / sr.orth_t: the same formulas).
    """
    import torch

    L, ctx = lib_ctx
    rs = np.random.RandomState(2000 + n)
    glued = sr.tridiagonal_inputs(n)["glued1e-4"]
    e_random = rs.randn(n)
    e_random[n - 1] = 0.0
    names = ["random", "glued1e-4"]
    d = np.stack([rs.randn(n), glued[0]])
    e = np.stack([e_random, glued[1]])
    w, z = sr.stedc_host(L, ctx, d, e)
    rows = []
    for b, name in enumerate(names):
        t, zb, wb = (torch.from_numpy(x).cuda() for x in (sr.tridiagonal(d[b], e[b]), z[b], w[b]))
        assert np.all(np.diff(w[b]) >= 0.0), (name, "eigenvalues not ascending")
        rows.append((name, {"recon(T,Z,w)": sr.recon_t(t, zb, torch.diag(wb)), "orth(Z)": sr.orth_t(zb)}))
    report(f"stedc n={n} thresholds", rows)


# ---- the staged entries against the product path ---------------------------------------------------------------------------
@pytest.mark.parametrize("two_stage,n", [(True, 322), (False, 322)])
def test_stages_compose_to_the_product(lib_ctx, two_stage, n):
    """
    V of sc_dev_eigh_f64 against (Q Z)^T built from the two staged entries, for a batch of two (the batched kernels on
    both paths): |V - (Q Z)^T|_1 <= 50 n ulp, and the eigenvalues agree to 50 n ulp lambda_max.  Ties the stages to the
    product.
    """
    import torch

    L, ctx = lib_ctx
    mats = np.stack([sr.random_sym(n), sr.mixed_batch(n)[1][sr.MIXED.index("band65")]])
    ctx.set_two_stage(two_stage)
    a = torch.from_numpy(mats.copy()).cuda()
    w = torch.empty((2, n), dtype=torch.float64, device="cuda")
    v = torch.empty((2, n, n), dtype=torch.float64, device="cuda")
    ctx.check(L.sc_dev_eigh_f64(ctx.handle, C.c_void_p(a.data_ptr()), n, 2, C.c_void_p(w.data_ptr()),
                                C.c_void_p(v.data_ptr())))
    ctx.synchronize()
    w, v = w.cpu().numpy(), v.cpu().numpy()
    d, e, s, _, q, two = sr.reduce_host(L, ctx, mats, sr.Q_ALL)
    assert two == two_stage
    ws, z = sr.stedc_host(L, ctx, d, e)
    figures = []
    for b in range(2):
        diff = sr.norm1(v[b] - (q[b] @ z[b]).T) / (n * sr.ULP)
        eig = np.abs(w[b] - ws[b] / s[b]).max() / (np.abs(w[b]).max() * n * sr.ULP)
        figures.append((diff, eig))
        print(f"[compose two_stage={two_stage} n={n}] member {b}: |V - (Q Z)^T|_1 / (n ulp) = {diff:.3g}, "
              f"eigenvalue difference / (n ulp lambda_max) = {eig:.3g}")
    assert all(diff <= sr.GATE and eig <= sr.GATE for diff, eig in figures), figures


# ---- one kernel form per case, proven by the form counters ------------------------------------------------------------------
# Calls of run_panel by panel-QR form and by role, SYMM and trailing-update forms: per call of the staged entry.
PER_CALL = ("panel_coop_launches", "panel_wg1_launches", "panel_wg2_launches", "panel_wg3_launches", "panel_wg4_launches",
            "panel_wg10_launches", "panel_wg12_launches", "panel_blocked_launches", "panel_unblocked_launches",
            "panel_pair_first", "panel_pair_second", "symm3_launches", "symm_tri_launches", "gemm3_declined")
LAST = ("symm_slices", "stage1_parts", "chase_stream_parts")                   # of the most recent solve
BT2 = ("bt2_wave_solves", "bt2_apply4_solves", "bt2_apply8_solves", "bt2_xcd_launches")
QUIET = ("panel_coop_timeouts", "chase_timeouts", "chase_incomplete", "chase_resumed", "chase_pair_fallbacks")
# every switch of tools/test_matrix.sh that moves a shape to another form
FORM_SWITCHES = ("QR_UNBLOCKED", "QR_WG", "QR_COOP", "QR_COOP_MIN", "STAGE1_STREAMS", "PANEL_PAIRS", "SYMM3", "SYMM_SPLIT",
                 "GEMM3", "GEMM3_LOWER", "BULGE_PERSISTENT", "BULGE_STREAMS", "BULGE_PAIR", "BULGE_SPREAD", "BT2_WAVE", "BT2_NW")


def skip_if_forms_overridden():
    hit = [k for k in FORM_SWITCHES if os.environ.get("SPRINGCRAFT_" + k)]
    if hit:
        pytest.skip(f"the form under test is overridden by {hit} (tools/test_matrix.sh)")


def wrong_forms(ctx, label, calls, per_call, last, bt2, stepwise):
    """Every form counter against its literal: those named, and zero for all the others; prints them and returns the
    mismatches {counter: (got, expected)}."""
    got = {k: ctx.counter(k) for k in PER_CALL + LAST + BT2 + QUIET + ("chase_launches", "stepwise_chases", "gemm3_launches")}
    print(f"[{label}] call {calls}: " + " ".join(f"{k}={v}" for k, v in got.items() if v))
    assert set(per_call) <= set(PER_CALL) and set(last) == set(LAST) and set(bt2) <= set(BT2)
    want = {k: calls * per_call.get(k, 0) for k in PER_CALL}
    want.update(last)
    want.update({k: bt2.get(k, 0) for k in BT2})
    want.update({k: 0 for k in QUIET})
    want["chase_launches"], want["stepwise_chases"] = (0, calls) if stepwise else (calls, 0)
    return {k: (got[k], v) for k, v in want.items() if got[k] != v}


def check_forms(ctx, label, calls, per_call, last, bt2, stepwise):
    wrong = wrong_forms(ctx, label, calls, per_call, last, bt2, stepwise)
    assert not wrong, (label, "counter: (got, expected)", wrong)


def cycled_batch(n, batch, copies):
    """`batch` members of order n: random_sym(n) at the positions `copies`, the mixed batch's members in turn elsewhere."""
    _, mixed = sr.mixed_batch(n)
    names, mats = [], []
    for k in range(batch):
        if k in copies:
            names.append(f"copy@{k}")
            mats.append(sr.random_sym(n))
        else:
            names.append(f"{sr.MIXED[k % len(sr.MIXED)]}@{k}")
            mats.append(mixed[k % len(sr.MIXED)])
    return names, np.stack(mats)


def members_batch(n, names):
    if ("members", n, tuple(names)) not in sr._cache:
        members, _ = sr.degenerate_members(n, sr.SEED, names=names)
        by_name = dict(members)
        sr._cache["members", n, tuple(names)] = np.stack([by_name[k] for k in names])
    return [f"{k}@{i}" for i, k in enumerate(names)], sr._cache["members", n, tuple(names)]


def stage1_on_device(L, ctx, label, names, mats, per_call, slices):
    """which = Q_ONE of a large order: recon(A,Q1,B), orth(Q1) by the torch twins on the device, beyond_band."""
    import torch

    t0 = time.perf_counter()
    d, e, s, band, qt, two = sr.reduce_host(L, ctx, mats, sr.Q_ONE, transpose=False)
    t1 = time.perf_counter()
    assert two, "the two-stage path was forced"
    rows = []
    for b, name in enumerate(names):
        a = torch.from_numpy(scaled(mats[b], s[b])).cuda()
        q = torch.from_numpy(qt[b]).cuda().T          # (the entry returns the factor's columns as rows)
        bm = torch.from_numpy(sr.band_matrix(band[b])).cuda()
        rows.append((name, {"recon(A,Q1,B)": sr.recon_t(a, q, bm), "orth(Q1)": sr.orth_t(q),
                            "beyond_band": sr.band_beyond(band[b])}))
    print(f"[{label}] solve {t1 - t0:.2f} s, ratios {time.perf_counter() - t1:.2f} s")
    wrong = wrong_forms(ctx, label, 1, per_call, {"symm_slices": slices, "stage1_parts": 1, "chase_stream_parts": 0}, {}, False)
    report(label, rows)
    assert not wrong, (label, "counter: (got, expected)", wrong)


# (the literals: tests/host_sanitize/test_host_logic.cpp, shapes a .. h; k_symm3 takes a panel of m even rows while
# ceil(m / 128) x slices x matrices >= 256 and every slice has four K steps, k_gemm3 a trailing update of fewer than eight
# matrices while its lower triangle has 1024 tiles of 128 x 64 over the batch)
STAGE1_CASES = {
    # one matrix of 1036 rows: <2,8> once; 9 x 16 = 144 items: k_symm3 declines every panel, its 16 slices go through the
    # triangular-operand launches and k_sum_xslices over 2 x 64 columns
    "a": (1100, ["random"], False, dict(panel_wg2_launches=1, panel_wg1_launches=15, panel_unblocked_launches=1, panel_pair_first=6,
                                        panel_pair_second=6, symm_tri_launches=17, gemm3_declined=11), 16),
    # k_symm3 with 16 slices on the panels of 2056, 1992 and 1928 rows (17, 16, 16 tile rows)
    "b": (2120, ["random"], False, dict(panel_wg3_launches=1, panel_wg2_launches=16, panel_wg1_launches=15, panel_unblocked_launches=1,
                                        panel_pair_first=14, panel_pair_second=14, symm3_launches=3, symm_tri_launches=30,
                                        gemm3_declined=19), 16),
    "c": (3140, ["random"], False, dict(panel_wg4_launches=1, panel_wg3_launches=16, panel_wg2_launches=16, panel_wg1_launches=15,
                                        panel_unblocked_launches=1, panel_pair_first=22, panel_pair_second=22, symm3_launches=19,
                                        symm_tri_launches=30, gemm3_declined=27), 16),
    # (k_gemm3 takes the joint update of 4034 rows: 32 x 64 - 32 x 31 = 1056 tiles; 3906 rows have 992)
    "d": (4162, ["random"], False, dict(panel_blocked_launches=1, panel_wg4_launches=16, panel_wg3_launches=16, panel_wg2_launches=16,
                                        panel_wg1_launches=15, panel_unblocked_launches=1, panel_pair_first=30,
                                        panel_pair_second=30, symm3_launches=35, symm_tri_launches=30, gemm3_declined=34), 16),
    "e": (4162, ["random", "rank1", "gluedW", "big"], True,
          dict(panel_wg10_launches=1, panel_wg4_launches=16, panel_wg3_launches=16, panel_wg2_launches=16, panel_wg1_launches=15,
               panel_unblocked_launches=1, panel_pair_first=30, panel_pair_second=30, symm3_launches=55, symm_tri_launches=10,
               gemm3_declined=18), 12),
    "f": (5190, ["random", "rank1", "gluedW", "big"], True,
          dict(panel_wg12_launches=1, panel_wg10_launches=16, panel_wg4_launches=16, panel_wg3_launches=16, panel_wg2_launches=16,
               panel_wg1_launches=15, panel_unblocked_launches=1, panel_pair_first=38, panel_pair_second=38, symm3_launches=69,
               symm_tri_launches=12, gemm3_declined=18), 10),
    # odd order: no k_symm3, the triangular-operand launches with 9 slices on every panel; no 16-byte alignment: k_gemm3
    # declines all 17 trailing updates (31 panels, 14 of them first of a pair); one matrix: k_panel_coop from 300 rows
    "h": (2049, ["random"], True, dict(panel_coop_launches=27, panel_wg1_launches=4, panel_pair_first=14, panel_pair_second=14,
                                       symm_tri_launches=31, gemm3_declined=17), 9),
}


@pytest.mark.parametrize("case", sorted(STAGE1_CASES))
def test_form_stage1(lib_ctx, case):
    """
    Stage 1 alone (which = Q_ONE) at the smallest order that selects k_panel_wg<2,8> (a), <3,4> (b), <4,2> (c), the blocked
    chunked launches followed by every 1024-thread instance (d: one matrix of 4098 rows), <10,1,512> (e) and <12,1,512>
    (e, f: four matrices, random / rank1 / gluedW / big), and the triangular-operand SYMM with 9 K slices under trailing updates
    k_gemm3 declines (h: odd order).  a - d with k_panel_coop switched off, which would take their panels from 300 rows.
    """
    skip_if_forms_overridden()
    n, members, coop, per_call, slices = STAGE1_CASES[case]
    L, ctx = lib_ctx
    names, mats = (["random"], sr.random_sym(n)[None]) if members == ["random"] else members_batch(n, members)
    ctx.set_two_stage(True)
    if not coop:
        ctx.check(L.sc_dbg_set_panel_coop(ctx.handle, 0))
    stage1_on_device(L, ctx, f"form {case}: stage 1 n={n} x {len(names)}", names, mats, per_call, slices)


def identical(out, which, copies, label):
    first = copies[0]
    for k in copies[1:]:
        for x, what in zip(out[which][:5], ("d", "e", "scale", "band", "Q")):
            assert np.array_equal(x[k], x[first], equal_nan=True), (label, f"{what} of member {k} differs from member {first}'s")


def test_form_panel_pairs_on_the_mixed_batch(lib_ctx):
    """g: n = 450, the smallest order region with a panel pair (450 - 128 >= 256 > 450 - 256) on the members with tau = 0
    reflectors and exact zeros: record D, the Corr records and the K = 256 joint update; all three factors."""
    skip_if_forms_overridden()
    L, ctx = lib_ctx
    names, mats = sr.mixed_batch(450)
    ctx.set_two_stage(True)
    label = "form g: pairs n=450 mixed"
    per_call = dict(panel_wg1_launches=6, panel_unblocked_launches=1, panel_pair_first=1, panel_pair_second=1, symm_tri_launches=7,
                    gemm3_declined=6)

    def counters(calls):
        check_forms(ctx, label, calls, per_call, {"symm_slices": 1, "stage1_parts": 1, "chase_stream_parts": 0},
                    {"bt2_apply4_solves": calls - 1}, False)

    t0 = time.perf_counter()
    check_two_stage(L, ctx, label, names, mats, counters)
    print(f"[{label}] {time.perf_counter() - t0:.2f} s")


def test_form_two_stage1_parts(lib_ctx):
    """i: 33 matrices, the band reduction in two parts of 16 and 17 on two streams; one matrix at positions 0, 16 (the first
    of the second part) and 32: d, e, the band and Q1 of the three copies are bit-identical."""
    skip_if_forms_overridden()
    L, ctx = lib_ctx
    n, copies = 322, (0, 16, 32)
    names, mats = cycled_batch(n, 33, copies)
    ctx.set_two_stage(True)
    label = "form i: two stage-1 parts n=322 x 33"
    t0 = time.perf_counter()
    out = {sr.Q_ONE: sr.reduce_host(L, ctx, mats, sr.Q_ONE)}
    assert out[sr.Q_ONE][5]
    d, e, s, band, q1, _ = out[sr.Q_ONE]
    rows = [(name, {"recon(A,Q1,B)": sr.recon(scaled(mats[b], s[b]), q1[b], sr.band_matrix(band[b])), "orth(Q1)": sr.orth(q1[b]),
                    "beyond_band": sr.band_beyond(band[b])}) for b, name in enumerate(names)]
    print(f"[{label}] {time.perf_counter() - t0:.2f} s")
    wrong = wrong_forms(ctx, label, 1, dict(panel_wg1_launches=8, panel_unblocked_launches=2, symm_tri_launches=10,
                                            gemm3_declined=10),
                        {"symm_slices": 1, "stage1_parts": 2, "chase_stream_parts": 0}, {}, False)
    report(label, rows)
    assert not wrong, (label, "counter: (got, expected)", wrong)
    identical(out, sr.Q_ONE, copies, label)


@pytest.mark.parametrize("batch,parts,s1_parts,copies", [(16, 2, 1, (0, 8, 15)), (48, 3, 2, (0, 16, 32, 47))])
def test_form_stepwise_chase(lib_ctx, batch, parts, s1_parts, copies):
    """j: k_bulge_step, one launch per wavefront of tasks (sc_dbg_set_chase mode 0), the batch in two (16 matrices) and three
    (48) parts on separate streams; copies of one matrix in every part are bit-identical in all three factors."""
    skip_if_forms_overridden()
    L, ctx = lib_ctx
    n = 322
    names, mats = cycled_batch(n, batch, copies)
    ctx.set_two_stage(True)
    ctx.check(L.sc_dbg_set_chase(ctx.handle, 0, 0))
    label = f"form j: stepwise chase n={n} x {batch}"
    per_call = dict(panel_wg1_launches=4 * s1_parts, panel_unblocked_launches=s1_parts, symm_tri_launches=5 * s1_parts,
                    gemm3_declined=5 * s1_parts)

    def counters(calls):
        check_forms(ctx, label, calls, per_call, {"symm_slices": 1, "stage1_parts": s1_parts, "chase_stream_parts": parts},
                    {"bt2_apply4_solves": calls - 1, "bt2_xcd_launches": calls - 1}, True)

    t0 = time.perf_counter()
    out = check_two_stage(L, ctx, label, names, mats, counters)
    print(f"[{label}] {time.perf_counter() - t0:.2f} s")
    for which in (sr.Q_ONE, sr.Q_TWO, sr.Q_ALL):
        identical(out, which, copies, label)


@pytest.mark.parametrize("batch,nw", [(9, 4), (86, 8)])
def test_form_bt2_xcd_deal(lib_ctx, batch, nw):
    """k, l: the Q2 back-transformation with the workgroups dealt to the XCDs by matrix (eight matrices and more; neither batch a
    multiple of eight): k_bt2_apply<4> (9 matrices) and k_bt2_apply<8> (86: 3 x 86 = 258 workgroups of 128 columns reach the
    256 CUs; 85 would not).  Q2 alone and the whole factor (which = 0) of every member."""
    skip_if_forms_overridden()
    L, ctx = lib_ctx
    n = 322
    s1_parts = 2 if batch >= 32 else 1
    names, mats = cycled_batch(n, batch, (0,))
    ctx.set_two_stage(True)
    label = f"form {'k' if nw == 4 else 'l'}: bt2 XCD deal n={n} x {batch}"
    per_call = dict(panel_wg1_launches=4 * s1_parts, panel_unblocked_launches=s1_parts, symm_tri_launches=5 * s1_parts,
                    gemm3_declined=5 * s1_parts)
    t0 = time.perf_counter()
    out, wrong = {}, {}
    for calls, which in enumerate((sr.Q_TWO, sr.Q_ALL), 1):
        out[which] = sr.reduce_host(L, ctx, mats, which)
        assert out[which][5]
        wrong[calls] = wrong_forms(ctx, label, calls, per_call, {"symm_slices": 1, "stage1_parts": s1_parts, "chase_stream_parts": 0},
                                   {f"bt2_apply{nw}_solves": calls, "bt2_xcd_launches": calls}, False)
    rows = []
    for b, name in enumerate(names):
        d, e, s, band, q2, _ = (x[b] if isinstance(x, np.ndarray) else x for x in out[sr.Q_TWO])
        fig = {"recon(B,Q2,T)": sr.recon(sr.band_matrix(band), q2, sr.tridiagonal(d, e)), "orth(Q2)": sr.orth(q2),
               "beyond_band": sr.band_beyond(band)}
        d, e, s, band, q, _ = (x[b] if isinstance(x, np.ndarray) else x for x in out[sr.Q_ALL])
        fig["recon(A,Q,T)"] = sr.recon(scaled(mats[b], s), q, sr.tridiagonal(d, e))
        fig["orth(Q)"] = sr.orth(q)
        rows.append((name, fig))
    print(f"[{label}] {time.perf_counter() - t0:.2f} s")
    report(label, rows)
    assert not any(wrong.values()), (label, "call: counter: (got, expected)", wrong)


# ---- the band reduction's plan (csrc/sy2sb_plan.h): panel shapes, pairs and parts at the smallest orders that have them -----
# pairs of panels per matrix: panel_roles of tests/host_sanitize/test_sy2sb_plan.cpp (384: 1, 2, 0, 0, 0; 512 and 513: 1, 2, 1, 2,
# 0, 0, 0).  Below n = 256 the two-stage path does not exist (eigh_policy.h: two_stage_for): the staged entry refuses the
# order, and the panel shapes of 66, 128 and 129 -- two rows; 64 rows with 63 reflectors; 65 rows -- are the last panels of
# 322 (test_form_two_stage1_parts and others), 384 and 513.
PLAN_PAIRS = {66: None, 128: None, 129: None, 384: 1, 512: 2, 513: 2}


@pytest.mark.parametrize("batch", [1, 3, 33])
@pytest.mark.parametrize("n", sorted(PLAN_PAIRS))
def test_stage1_plan_orders(lib_ctx, n, batch):
    """
    Stage 1 (which = Q_ONE) with the two-stage path forced, one / three / 33 matrices: the stage-1 gates on every member, as
    many first and second panels of a pair as the roles say (per part), two parts of 16 and 17 matrices at batch 33 and
    one otherwise; at batch 33 the copies of one matrix at positions 0, 16 (the first of the second part) and 32 have
    bit-equal d, e, band and Q1 -- the rule at sc_host::stage1_parts.
    """
    skip_if_forms_overridden()
    L, ctx = lib_ctx
    copies = (0, 16, 32) if batch == 33 else (0,)
    ctx.set_two_stage(True)
    label = f"plan: stage 1 n={n} x {batch}"
    if PLAN_PAIRS[n] is None:
        rc, _ = sr.reduce_raw(L, ctx, np.stack([sr.random_sym(n)] * batch), sr.Q_ONE)
        assert rc == 1, rc          # SC_ERR_INVALID_ARG: below the two-stage minimum
        return
    names, mats = cycled_batch(n, batch, copies)
    t0 = time.perf_counter()
    out = {sr.Q_ONE: sr.reduce_host(L, ctx, mats, sr.Q_ONE)}
    d, e, s, band, q1, two = out[sr.Q_ONE]
    assert two, "the two-stage path was forced"
    rows = [(name, {"recon(A,Q1,B)": sr.recon(scaled(mats[b], s[b]), q1[b], sr.band_matrix(band[b])), "orth(Q1)": sr.orth(q1[b]),
                    "beyond_band": sr.band_beyond(band[b])}) for b, name in enumerate(names)]
    got = {k: ctx.counter(k) for k in PER_CALL + LAST + QUIET}
    print(f"[{label}] {time.perf_counter() - t0:.2f} s  " + " ".join(f"{k}={v}" for k, v in got.items() if v))
    report(label, rows)
    parts = 2 if batch == 33 else 1
    assert got["stage1_parts"] == parts, got
    assert got["panel_pair_first"] == PLAN_PAIRS[n] * parts and got["panel_pair_second"] == PLAN_PAIRS[n] * parts, got
    assert all(got[k] == 0 for k in QUIET), got
    identical(out, sr.Q_ONE, copies, label)


def test_stage1_plan_coop(lib_ctx):
    """k_panel_coop through the plan's carve of the auxiliary buffer: n = 384, one matrix, panels of at least 200 rows (320 and
    256: the two panels of the pair), two workgroups each."""
    skip_if_forms_overridden()
    if coop_overridden():
        pytest.skip("the cooperative kernel's rule is overridden (tools/test_matrix.sh)")
    L, ctx = lib_ctx
    n = 384
    mats = sr.random_sym(n)[None]
    ctx.set_two_stage(True)
    ctx.check(L.sc_dbg_set_panel_coop(ctx.handle, 200))
    label = f"plan: k_panel_coop n={n} x 1"
    d, e, s, band, q1, two = sr.reduce_host(L, ctx, mats, sr.Q_ONE)
    assert two, "the two-stage path was forced"
    got = {k: ctx.counter(k) for k in PER_CALL + LAST + QUIET}
    print(f"[{label}] " + " ".join(f"{k}={v}" for k, v in got.items() if v))
    report(label, [("random", {"recon(A,Q1,B)": sr.recon(scaled(mats[0], s[0]), q1[0], sr.band_matrix(band[0])),
                               "orth(Q1)": sr.orth(q1[0]), "beyond_band": sr.band_beyond(band[0])})])
    assert got["panel_coop_launches"] == 2 and got["panel_pair_first"] == 1 and got["panel_pair_second"] == 1, got
    assert got["stage1_parts"] == 1 and all(got[k] == 0 for k in QUIET), got
