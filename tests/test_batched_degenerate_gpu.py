"""
GPU parity tests of the batched full-spectrum solve (``sc_dev_eigh_f64``: what ``DeviceBatchSolver`` and
``RaggedBatchSolver`` call and ``bench.py`` times) on batches of MIXED, DEGENERATE members -- tests.util.degenerate_members:
identity, zero, diagonal, tridiagonal, banded inside / at / just outside the stage-1 band, block diagonal, rank one,
exact and near multiplicities, graded, glued Wilkinson, extreme scales, an integer Kirchhoff matrix -- next to a random
control.  A single matrix takes other kernels than a batch, so these members reach the batch's kernels only here: the
batched launch-per-column tridiagonalisation, k_panel_wg / k_panel_coop / k_panel_serial on panels whose columns are
exactly zero, k_symm3 and the lower-only k_gemm3 with V = 0 for some members, k_bulge_pair / k_bulge_chase with reflectors
tau = 0 (both forms, the spread form, the give-up write-back and the take-over), the decoupled-columns branch of
k_dia_tfactor2, the batched D&C with every pole of one member deflated next to members with none, and the per-matrix
power-of-two scaling of a full-spectrum batch.

Every case is ONE batched solve (the placement case: three) on a private context, path and kernel form forced as in
tests/test_two_stage_gpu.py and confirmed by the context's counters.  EVERY member is checked, with the gates the project
pins for batched solves: eigenvalues against LAPACK (and the closed form where the zoo has one) to 1e-11 max(lambda_max,
tiny); residual max|A V^T - V^T diag(w)| <= 1e-10 max(lambda_max, 1) on the device (`big` / `small`: relative to their own
lambda_max); ||V V^T - I||_max <= 1e-11.  (tests/test_batched_degenerate_host.py: LAPACK meets each with a factor > 100.)
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import degenerate_members

pytestmark = pytest.mark.gpu

SEED = 1
ZOO = ["random", "identity", "zero", "diag", "tridiag", "band40", "band64", "band65", "blockdiag", "rank1", "clustered",
       "nearclustered", "graded", "gluedW", "big", "small", "kirchhoff"]
TINY = 1e-300

_members, _exact, _lapack = {}, {}, {}


def member(n, name):
    """(a, LAPACK's eigenvalues, exact spectrum or None) of one member; built once per module run, read-only."""
    if (n, name) not in _members:
        members, exact = degenerate_members(n, SEED, names=[name])
        a = members[0][1]
        a.setflags(write=False)
        _members[n, name] = a
        _exact[n, name] = exact.get(name)
        _lapack[n, name] = np.linalg.eigvalsh(a)
    return _members[n, name], _lapack[n, name], _exact[n, name]


def debug_lib():
    from springcraft_amd import _hip

    L = _hip.lib()
    L.sc_dbg_set_chase.restype = C.c_int
    L.sc_dbg_set_chase.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for f in (L.sc_dbg_set_panel_coop, L.sc_dbg_set_panel_coop_fail):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int]
    return L


def solve(ctx, L, n, names, vectors=True):
    """One batched solve of the named members, in that order: (w, v or None) on the device."""
    import torch

    batch = len(names)
    a = torch.from_numpy(np.stack([member(n, name)[0] for name in names])).cuda()
    w = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    v = torch.empty((batch, n, n), dtype=torch.float64, device="cuda") if vectors else None
    ctx.check(L.sc_dev_eigh_f64(ctx.handle, C.c_void_p(a.data_ptr()), n, batch, C.c_void_p(w.data_ptr()),
                                C.c_void_p(v.data_ptr()) if vectors else None))
    ctx.synchronize()
    return w, v


def check_members(label, n, names, w, v):
    """Every member against the three gates; the figures are printed before anything is asserted."""
    import torch

    wh = w.cpu().numpy()
    rows, failures = [], []
    eye = torch.eye(n, dtype=torch.float64, device="cuda") if v is not None else None
    for b, name in enumerate(names):
        a, w_ref, exact = member(n, name)
        lam = np.abs(w_ref).max()
        finite = bool(np.isfinite(wh[b]).all()) and (v is None or bool(torch.isfinite(v[b]).all()))
        eig = np.abs(wh[b] - w_ref).max()
        if exact is not None:
            eig = max(eig, np.abs(wh[b] - exact).max())
        eig_gate = 1e-11 * max(lam, TINY)
        res = orth = 0.0
        res_gate = 1e-10 * (lam if name in ("big", "small") else max(lam, 1.0))
        if v is not None and finite:
            ad = torch.from_numpy(a.copy()).cuda()   # (the cached member is read-only)
            res = float((ad @ v[b].T - v[b].T * w[b][None, :]).abs().max())
            orth = float((v[b] @ v[b].T - eye).abs().max())
        rows.append((name, eig / max(lam, TINY), res / (res_gate / 1e-10), orth))
        if not finite:
            failures.append((name, "not finite"))
        if not eig <= eig_gate:
            failures.append((name, "eigenvalues", eig, eig_gate))
        if not res <= res_gate:
            failures.append((name, "residual", res, res_gate))
        if not orth <= 1e-11:
            failures.append((name, "orthogonality", orth))
    worst = [max(rows, key=lambda r: r[k]) for k in (1, 2, 3)]
    print(f"\n[{label}] worst eigenvalue error {worst[0][1]:.2e} ({worst[0][0]}), residual {worst[1][2]:.2e} "
          f"({worst[1][0]}), orthogonality {worst[2][3]:.2e} ({worst[2][0]})")
    for r in rows:
        print(f"[{label}]   {r[0]:<14s} eig {r[1]:.2e}  res {r[2]:.2e}  orth {r[3]:.2e}")
    # `big` and `small` are `random` times 1e150 / 1e-150: the per-matrix power-of-two scaling must give the same
    # eigenvalues but for that factor (1e-12 of lambda_max: the products a * 1e150 are rounded, an ulp per entry)
    if "random" in names:
        w0 = wh[names.index("random")]
        for name, factor in (("big", 1e150), ("small", 1e-150)):
            if name in names:
                d = np.abs(wh[names.index(name)] - factor * w0).max() / (factor * np.abs(w0).max())
                print(f"[{label}]   {name} against {factor:g} * random: {d:.2e}")
                if not d <= 1e-12:
                    failures.append((name, "scaling", d))
    assert not failures, failures


def chase_counters(ctx):
    return {k: ctx.counter(k) for k in ("chase_launches", "chase_timeouts", "chase_incomplete", "chase_resumed",
                                        "chase_sweeps", "stepwise_chases", "chase_pair_launches", "chase_pair_fallbacks",
                                        "chase_xcd_max", "chase_xcd_total", "xcd_count")}


def check_chase(cnt, form, give_up, n, batch, solves=1):
    """The counters test_persistent_chase_and_resume asserts: one launch in the form that was asked for, no time-out."""
    assert cnt["chase_launches"] == solves and cnt["stepwise_chases"] == 0, cnt
    assert cnt["chase_pair_launches"] == (solves if form == 3 else 0) and cnt["chase_pair_fallbacks"] == 0, cnt
    assert cnt["chase_timeouts"] == 0 and cnt["chase_incomplete"] == 0, cnt
    if give_up == 0:
        assert cnt["chase_resumed"] == 0 and cnt["chase_sweeps"] == solves * batch * (n - 2), cnt
    else:
        assert cnt["chase_resumed"] == solves and cnt["chase_sweeps"] < solves * batch * (n - 2), cnt
    if form == 5:
        # the spread form draws its tickets from ONE slot (every workgroup counts as XCD 0), the others from one per XCD
        assert cnt["xcd_count"] > batch and cnt["chase_xcd_total"] == cnt["chase_xcd_max"] > 0, cnt
    else:
        assert cnt["chase_xcd_total"] > cnt["chase_xcd_max"], cnt


@pytest.mark.parametrize("n", [322, 513])
def test_one_stage_whole_zoo(n):
    """The batched launch-per-column tridiagonalisation, the batched D&C and the Q1 back-transformation."""
    from springcraft_amd import _hip

    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(False)
        w, v = solve(ctx, L, n, ZOO)
        cnt = chase_counters(ctx)
        assert cnt["chase_launches"] == 0 and cnt["stepwise_chases"] == 0, cnt      # stage 2 did not run: one-stage
        assert ctx.counter("resident_launches") == 0                               # (nor the single solve's kernel)
        check_members(f"one-stage n={n}", n, ZOO, w, v)
    finally:
        ctx.close()


@pytest.mark.parametrize("n,give_up", [(322, 0), (1030, 0), (1030, 5)])
@pytest.mark.parametrize("form", [3, 4])
def test_two_stage_whole_zoo(n, give_up, form):
    """
    Stage 1 by k_panel_wg, the persistent chase in the pair form (3: k_bulge_pair) and with one sweep per workgroup (4:
    k_bulge_chase), n = 322 with partial last blocks; give_up 5: every workgroup gives up after five tasks -- the pair
    form's write-back of its LDS slots -- and k_chase_finish takes the chase over.
    """
    from springcraft_amd import _hip

    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(True)
        ctx.check(L.sc_dbg_set_chase(ctx.handle, form, give_up))
        w, v = solve(ctx, L, n, ZOO)
        check_chase(chase_counters(ctx), form, give_up, n, len(ZOO))
        check_members(f"two-stage n={n} form={form} give_up={give_up}", n, ZOO, w, v)
    finally:
        ctx.close()


def test_two_stage_spread_chase():
    """Form 5 (k_bulge_chase<1>: the workgroups of a matrix on all XCDs) takes fewer matrices than the device has XCDs."""
    from springcraft_amd import _hip

    n, names = 1030, ["random", "identity", "blockdiag", "band65", "gluedW", "big"]
    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(True)
        ctx.check(L.sc_dbg_set_chase(ctx.handle, 5, 0))
        w, v = solve(ctx, L, n, names)
        check_chase(chase_counters(ctx), 5, 0, n, len(names))
        check_members(f"two-stage n={n} form=5", n, names, w, v)
    finally:
        ctx.close()


@pytest.mark.parametrize("fail_panel", [-1, 2])
def test_cooperative_panel_and_take_over(fail_panel):
    """
    k_panel_coop on panels of exactly zero columns (`zero`; `blockdiag` below its first block) next to a random member,
    and with the hook k_panel_serial behind it from panel 2 on.
    """
    from springcraft_amd import _hip

    if os.environ.get("SPRINGCRAFT_QR_COOP") == "0" or os.environ.get("SPRINGCRAFT_QR_COOP_MIN") or \
            int(os.environ.get("SPRINGCRAFT_STAGE1_STREAMS") or 0) > 1:
        pytest.skip("the cooperative kernel's rule is overridden (tools/test_matrix.sh)")
    n, names = 1030, ["zero", "blockdiag", "random"]
    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(True)
        ctx.check(L.sc_dbg_set_panel_coop(ctx.handle, 200))
        ctx.check(L.sc_dbg_set_panel_coop_fail(ctx.handle, fail_panel))
        w, v = solve(ctx, L, n, names)
        launches, timeouts = ctx.counter("panel_coop_launches"), ctx.counter("panel_coop_timeouts")
        assert launches > 0, launches
        assert (timeouts == 0) if fail_panel < 0 else (timeouts > 0), timeouts
        check_members(f"cooperative panel n={n} fail_panel={fail_panel}", n, names, w, v)
    finally:
        ctx.close()


def test_symm3_and_lower_gemm3_in_a_batch():
    """4 x n = 2000, the smallest shape that runs k_symm3 in a batch: members whose V is zero in part or all of a panel."""
    from springcraft_amd import _hip

    if os.environ.get("SPRINGCRAFT_SYMM_SPLIT") or os.environ.get("SPRINGCRAFT_SYMM3") == "0":
        pytest.skip("the slice rule / the kernel choice is overridden (tools/test_matrix.sh)")
    n, names = 2000, ["random", "blockdiag", "clustered", "band65"]
    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(True)
        w, v = solve(ctx, L, n, names)
        assert ctx.counter("symm3_launches") > 0
        check_members(f"symm3 n={n}", n, names, w, v)
    finally:
        ctx.close()


@pytest.mark.parametrize("two_stage", [False, True])
def test_values_only_whole_zoo(two_stage):
    """The same entry without an eigenvector buffer, as DeviceBatchSolver(want_vectors=False) calls it."""
    from springcraft_amd import _hip

    n = 322
    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(two_stage)
        w, _ = solve(ctx, L, n, ZOO, vectors=False)
        cnt = chase_counters(ctx)
        assert cnt["chase_launches"] + cnt["stepwise_chases"] == (1 if two_stage else 0), cnt
        check_members(f"values only n={n} two_stage={two_stage}", n, ZOO, w, None)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", [3, 4])
def test_placement_in_the_batch(form):
    """
    A member's result must not depend on its place in the batch (the chase binds matrix b to XCD b mod 8; the D&C's
    GemmDesc records are laid out member by member): the same order again reproduces every bit, the reversed order agrees per
    member to 1e-12 lambda_max (the bound of test_reproducible_and_independent_of_the_shard_size).  Whether the reversed
    order is bit-equal too is printed, not asserted.
    """
    from springcraft_amd import _hip

    n = 322
    L = debug_lib()
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(True)
        ctx.check(L.sc_dbg_set_chase(ctx.handle, form, 0))
        w0, v0 = (t.cpu().numpy() for t in solve(ctx, L, n, ZOO))
        w1, v1 = (t.cpu().numpy() for t in solve(ctx, L, n, ZOO))
        wr, vr = solve(ctx, L, n, ZOO[::-1])
        check_chase(chase_counters(ctx), form, 0, n, len(ZOO), solves=3)
        assert np.array_equal(w0, w1) and np.array_equal(v0, v1)
        check_members(f"reversed order n={n} form={form}", n, ZOO[::-1], wr, vr)
        wr, vr = wr.cpu().numpy()[::-1], vr.cpu().numpy()[::-1]
        w_same = [name for b, name in enumerate(ZOO) if np.array_equal(w0[b], wr[b])]
        v_same = [name for b, name in enumerate(ZOO) if np.array_equal(v0[b], vr[b])]
        print(f"[reversed order n={n} form={form}] eigenvalues bit-equal for {len(w_same)} of {len(ZOO)} members, "
              f"eigenvectors for {len(v_same)}; not bit-equal: w {sorted(set(ZOO) - set(w_same))}, "
              f"v {sorted(set(ZOO) - set(v_same))}")
        for b, name in enumerate(ZOO):
            lam = np.abs(member(n, name)[1]).max()
            assert np.abs(wr[b] - w0[b]).max() <= 1e-12 * lam, (name, np.abs(wr[b] - w0[b]).max(), lam)
    finally:
        ctx.close()
