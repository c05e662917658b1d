"""
GPU tests of the device Cholesky solver (csrc/potrf.hip) through its C entries ``sc_dev_potrf_f64`` / ``sc_dev_potrs_f64`` on
torch tensors.

Orders 1, 2, 15 .. 17 (an MFMA tile edge), 63 .. 65 and 127 / 129 (the inner block of 64 columns), 200, 513 and 1030 (two
and three outer blocks of 512 columns, the last one a single column / a short inner block).  Inputs: ``Q diag(lambda) Q^T`` with condition numbers
1, 1e6 and 1e12 (tests/subsystem_model.py).  A torch tensor (n, n) is row-major; the solver reads the LOWER triangle of the
column-major matrix in the same buffer, that is the tensor's upper triangle: the tests fill the tensor's strict LOWER
triangle with NaN to see that the solver never writes it and that nothing depends on it.

Ratios are LAPACK's (dpot01, dpot02, dtrt02) in units of n ulp, gate 50 as for the eigensolver's stages (tests/stage_ratios.py);
NumPy's own factor reaches 0.001 .. 0.06 on these inputs.
"""
import ctypes as C

import numpy as np
import pytest

from tests import subsystem_model as sm

pytestmark = pytest.mark.gpu

SC_OK, SC_ERR_INVALID_ARG, SC_ERR_NOCONV = 0, 1, 7
FORWARD, BACKWARD, BOTH = 0, 1, 2


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def hip(torch):
    from springcraft_amd import _hip

    ctx = _hip.Context(torch.cuda.current_device(), stream=torch.cuda.current_stream().cuda_stream)
    yield _hip.lib(), ctx
    ctx.close()


def p(t):
    return C.c_void_p(t.data_ptr())


def packed(torch, mats, ld=None, gap=0):
    """(batch, ld, ld) CUDA buffer, matrix b in [b, :n, :n] with its strict lower triangle (the solver's upper one) NaN."""
    n = len(mats[0])
    ld = n if ld is None else ld
    buf = np.full((len(mats), ld + gap, ld), np.nan)
    for b, a in enumerate(mats):
        buf[b, :n, :n] = np.triu(a) + np.tril(np.full((n, n), np.nan), -1)
    return torch.from_numpy(buf).cuda()


def potrf(torch, hip, buf, n):
    L, ctx = hip
    batch, rows, ld = buf.shape
    info = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
    rc = L.sc_dev_potrf_f64(ctx.handle, p(buf), n, ld, rows * ld, batch, p(info))
    assert rc == SC_OK, L.sc_last_error(ctx.handle)
    return info


def factor_of(buf, b, n):
    """The factor L (n, n) lower of matrix b, and the part of the buffer the solver must not have written."""
    host = buf[b].cpu().numpy()
    return np.triu(host[:n, :n]).T, host


def check_untouched(host, n):
    low = np.tril_indices(n, -1)
    assert np.isnan(host[:n, :n][low]).all(), "the strict upper triangle of the column-major matrix was written"
    assert np.isnan(host[n:]).all() and np.isnan(host[:, n:]).all(), "the padding was written"


def potrs(torch, hip, buf, n, rhs, mode, ldb=None):
    """rhs (batch, q, n) host -> solutions (batch, q, n); the right-hand sides lie in rows of length ldb."""
    L, ctx = hip
    batch, rows, ld = buf.shape
    q = rhs.shape[1]
    ldb = n if ldb is None else ldb
    host = np.full((batch, q, ldb), np.nan)
    host[:, :, :n] = rhs
    dev = torch.from_numpy(host).cuda()
    rc = L.sc_dev_potrs_f64(ctx.handle, p(buf), n, ld, rows * ld, batch, p(dev), q, ldb, q * ldb, mode)
    assert rc == SC_OK, L.sc_last_error(ctx.handle)
    out = dev.cpu().numpy()
    assert np.isnan(out[:, :, n:]).all()
    return out[:, :, :n]


@pytest.mark.parametrize("cond", sm.POTRF_CONDS)
@pytest.mark.parametrize("n", sm.POTRF_ORDERS)
def test_factor_and_solves(torch, hip, n, cond):
    a = sm.spd(n, cond)
    buf = packed(torch, [a])
    info = potrf(torch, hip, buf, n)
    hip[1].synchronize()
    assert info.cpu().tolist() == [0]
    l, host = factor_of(buf, 0, n)
    check_untouched(host, n)
    r = sm.factor_ratio(a, l)
    print(f"n = {n} cond = {cond:g}: factor ratio {r:.3f}")
    assert np.isfinite(l).all() and r <= sm.RATIO_GATE
    rs = np.random.RandomState(n)
    for q in sm.POTRS_Q:
        b = rs.randn(q, n)
        x = potrs(torch, hip, buf, n, b[None], BOTH)[0]
        y = potrs(torch, hip, buf, n, b[None], FORWARD)[0]
        z = potrs(torch, hip, buf, n, b[None], BACKWARD)[0]
        ratios = (sm.solve_ratio(a, x.T, b.T), sm.triangular_ratio(l, y.T, b.T), sm.triangular_ratio(l.T, z.T, b.T))
        print(f"  q = {q}: both {ratios[0]:.3f} forward {ratios[1]:.3f} backward {ratios[2]:.3f}")
        assert max(ratios) <= sm.RATIO_GATE
        # `both` is the two passes one after the other, bit for bit
        assert np.array_equal(potrs(torch, hip, buf, n, y[None], BACKWARD)[0], x)
    hip[1].synchronize()


@pytest.mark.parametrize("n", [17, 65, 200, 513])
def test_batch_stride_and_leading_dimension(torch, hip, n):
    mats = [sm.spd(n, c, seed) for seed, c in enumerate((1e6, 1.0, 1e12))]
    single = []
    rs = np.random.RandomState(7)
    rhs = rs.randn(3, 5, n)
    for b, a in enumerate(mats):
        buf = packed(torch, [a])
        potrf(torch, hip, buf, n)
        single.append((factor_of(buf, 0, n)[0], potrs(torch, hip, buf, n, rhs[b][None], BOTH)[0]))
    buf = packed(torch, mats, ld=n + 3, gap=2)
    info = potrf(torch, hip, buf, n)
    x = potrs(torch, hip, buf, n, rhs, BOTH, ldb=n + 5)
    hip[1].synchronize()
    assert info.cpu().tolist() == [0, 0, 0]
    for b in range(3):
        l, host = factor_of(buf, b, n)
        check_untouched(host, n)
        assert np.array_equal(l, single[b][0]), f"matrix {b} differs from its batch-of-one factor"
        assert np.array_equal(x[b], single[b][1]), f"matrix {b} differs from its batch-of-one solve"


def broken(n, column, kind):
    """An SPD matrix changed so that the factorisation fails exactly at `column`."""
    a = np.array(sm.spd(n, 1e6, seed=9))
    if kind == "nan":
        a[column, column] = np.nan
        return a
    # the pivot of `column` is a[c, c] - |L[c, :c]|^2: lower the diagonal entry by twice the pivot
    l = np.linalg.cholesky(a)
    a[column, column] -= 2.0 * l[column, column] ** 2
    return a


@pytest.mark.parametrize("column, kind", [(0, "negative"), (70, "negative"), (199, "negative"), (70, "nan")])
def test_failed_member(torch, hip, column, kind):
    n = 200
    L, ctx = hip
    good = [sm.spd(n, 1e6, seed=1), sm.spd(n, 1.0, seed=2)]
    clean = []
    rhs = np.random.RandomState(3).randn(3, 2, n)
    for b, a in zip((0, 2), good):
        buf = packed(torch, [a])
        potrf(torch, hip, buf, n)
        clean.append((factor_of(buf, 0, n)[0], potrs(torch, hip, buf, n, rhs[b][None], BOTH)[0]))
    ctx.synchronize()
    buf = packed(torch, [good[0], broken(n, column, kind), good[1]])
    info = potrf(torch, hip, buf, n)
    x = potrs(torch, hip, buf, n, rhs, BOTH)
    assert L.sc_ctx_synchronize(ctx.handle) == SC_ERR_NOCONV
    assert b"positive definite" in L.sc_last_error(ctx.handle)
    assert L.sc_ctx_synchronize(ctx.handle) == SC_OK
    assert info.cpu().tolist() == [0, column + 1, 0]
    l, host = factor_of(buf, 1, n)
    check_untouched(host, n)
    assert np.isnan(l[np.tril_indices(n)]).all(), "the factor of the failed matrix is not NaN everywhere"
    assert np.isnan(x[1]).all()
    for b, (l_ref, x_ref) in zip((0, 2), clean):
        assert np.array_equal(factor_of(buf, b, n)[0], l_ref) and np.array_equal(x[b], x_ref)
    with pytest.raises(np.linalg.LinAlgError):   # the Python layer's mapping of the same status
        potrf(torch, hip, packed(torch, [broken(n, column, kind)]), n)
        ctx.synchronize()
    ctx.synchronize()


def test_argument_errors_return_before_a_launch(torch, hip):
    L, ctx = hip
    a = torch.eye(4, dtype=torch.float64, device="cuda")
    before = a.clone()
    info = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    b = torch.ones((1, 4), dtype=torch.float64, device="cuda")
    bad = [
        L.sc_dev_potrf_f64(ctx.handle, p(a), 0, 4, 16, 1, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, p(a), -1, 4, 16, 1, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, p(a), 4, 3, 16, 1, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, p(a), 4, 4, 16, 0, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, p(a), 2, 2, 3, 2, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, None, 4, 4, 16, 1, p(info)),
        L.sc_dev_potrf_f64(ctx.handle, p(a), 4, 4, 16, 1, None),
        L.sc_dev_potrf_f64(None, p(a), 4, 4, 16, 1, p(info)),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, p(b), 1, 4, 4, 3),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, p(b), 1, 4, 4, -1),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, p(b), -1, 4, 4, BOTH),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, p(b), 1, 3, 4, BOTH),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 0, 4, 16, 1, p(b), 1, 4, 4, BOTH),
        L.sc_dev_potrs_f64(ctx.handle, None, 4, 4, 16, 1, p(b), 1, 4, 4, BOTH),
        L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, None, 1, 4, 4, BOTH),
    ]
    assert bad == [SC_ERR_INVALID_ARG] * len(bad)
    size = C.c_size_t(0)
    assert L.sc_dev_potrf_workspace(0, 1, C.byref(size)) == SC_ERR_INVALID_ARG
    assert L.sc_dev_potrf_workspace(4, 1, None) == SC_ERR_INVALID_ARG
    assert L.sc_dev_potrf_workspace(1030, 3, C.byref(size)) == SC_OK and size.value > 3 * 1030 * 64 * 8
    assert L.sc_dev_potrs_f64(ctx.handle, p(a), 4, 4, 16, 1, None, 0, 4, 4, BOTH) == SC_OK   # no right-hand side: nothing to do
    ctx.synchronize()
    assert torch.equal(a, before) and info.cpu().tolist() == [-1] and bool((b == 1).all())
