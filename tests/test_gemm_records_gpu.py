"""
GPU unit tests of k_gemm2's record-level launches (springcraft_amd/csrc/gemm_f64.hip) through sc_dbg_gemm_records_host:
triangular operands (a_tri), gather lists (a_kidx, b_kidx, c_jidx), grouped launches of records of different sizes, the
XCD-paired launch with a ragged group count, sub-matrix views, lower_only with offsets, record lists longer than one grid.
The reference is the NumPy model of tests/gemm_records.py (checked on its own in tests/test_gemm_records_host.py).

Every launch is checked three ways:
  (a) outside the entries the model says the launch may write, the arena comes back bit for bit (the gaps, the padding
      up to the leading dimension, entries above the diagonal and other records' operands hold NaN or old values);
  (b) inside, the result is finite and within 4 eps max(K, 1) (|alpha| + |beta| + 1) of the model;
  (c) where a test says so, the stored entries equal those of a plain launch with the same block tile on operands the
      host masked or gathered: the K steps a triangular launch skips or masks add exact zeros and the others run in the
      same order, and a gather launch multiplies the same numbers in the same order.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.gemm_records import (AkBk, AmBk, AmBn, REC, ArenaBuilder, gemm_records_reference, positions, record, records,
                                same_bits, split_chunk, sum_slices, tri_keep)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# (layout, tile id) of the triangular instantiations: 11 = 128 x 128 (not for two k-contiguous operands), 12 = 128 x 64,
# 13 = 64 x 64
TRI_KERNELS = [(AmBk, 11), (AmBk, 12), (AmBk, 13), (AkBk, 12), (AkBk, 13)]


@pytest.fixture(scope="module")
def launch():
    from springcraft_amd import _hip

    L = _hip.lib()
    ctx = _hip.context()
    fn = L.sc_dbg_gemm_records_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p] + [C.c_int] * 9

    def run(arena, idx, recs, max_m, max_n, layout, tile, split_k=1, gather=0, tri=0, lower_grid=0, expect=0):
        """One launch on a copy of the arena: the arena as the launch left it."""
        recs = np.ascontiguousarray(recs, dtype=REC) if isinstance(recs, np.ndarray) else records(recs)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.array(arena, dtype=np.float64, copy=True)
        rc = fn(ctx.handle, out.ctypes.data, out.size, idx.ctypes.data, idx.size, recs.ctypes.data, len(recs), max_m, max_n,
                split_k, gather, tri, layout, lower_grid, tile)
        assert rc == expect, (rc, expect)
        return out

    return run


def check(out, arena, idx, recs, split_k=1, what=None):
    """Checks (a) and (b); returns the model's (expected arena, write mask)."""
    exp, mask, bound = gemm_records_reference(arena, idx, recs, split_k, with_bound=True)
    stray = ~mask & ~same_bits(out, arena)
    assert not stray.any(), (what, "written outside the records' entries", np.flatnonzero(stray)[:8])
    assert np.isfinite(out[mask]).all(), (what, "NaN or Inf stored", np.flatnonzero(mask & ~np.isfinite(out))[:8])
    over = np.abs(out[mask] - exp[mask]) > bound[mask]
    assert not over.any(), (what, float(np.abs(out[mask] - exp[mask]).max()), float(bound[mask].min()))
    return exp, mask


# ---- triangular operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,tile", TRI_KERNELS)
@pytest.mark.parametrize("a_tri", [1, 2])
def test_triangular_one_record(launch, a_tri, layout, tile):
    """A(i, k) counts for i >= k (1) or k > i (2): A and C are views into larger matrices, the excluded part of A is NaN.
    Equal to the plain launch on A with the excluded part set to 0."""
    shapes = [(m, m) for m in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 257)] + [(200, 130), (130, 200)]
    for (m, k), n, beta in itertools.product(shapes, (1, 64, 65), (0.0, 1.0)):
        bld = ArenaBuilder(m + 3 * k + n)
        r = bld.gemm(m, n, k, layout, alpha=-1.0 if beta else 1.0, beta=beta, a_tri=a_tri, pad_a=7, pad_b=3, pad_c=5)
        arena, idx = bld.finish()
        what = (a_tri, layout, tile, m, n, k, beta)
        out = launch(arena, idx, [r], m, n, layout, tile, tri=1)
        _, mask = check(out, arena, idx, [r], what=what)
        zeroed = arena.copy()
        zeroed[positions(r, idx)[0][~tri_keep(a_tri, m, k)]] = 0.0
        plain = r.copy()
        plain["a_tri"] = 0
        out0 = launch(zeroed, idx, [plain], m, n, layout, tile)
        assert np.array_equal(out[mask], out0[mask]), (what, float(np.abs(out[mask] - out0[mask]).max()))


@pytest.mark.parametrize("layout,tile", TRI_KERNELS)
@pytest.mark.parametrize("a_tri", [(1, 1, 1, 1), (2, 2, 2, 2), (0, 1, 0, 1), (2, 0, 1, 2)])
def test_triangular_grouped_panels(launch, a_tri, layout, tile):
    """Four records shaped like consecutive panels of the band reduction under one max_m: the tiles of all records are
    dealt longest first, the row tiles of a_tri = 1 records in reverse order.  Also with a_tri = 0 records among them."""
    bld = ArenaBuilder(tile + layout)
    recs = [bld.gemm(m, 64, m, layout, alpha=-1.0, beta=1.0 if t % 2 else 0.0, a_tri=a_tri[t], pad_a=7, pad_c=5)
            for t, m in enumerate((300, 236, 172, 108))]
    arena, idx = bld.finish()
    out = launch(arena, idx, recs, 300, 64, layout, tile, tri=1)
    check(out, arena, idx, recs, what=(a_tri, layout, tile))


@pytest.mark.parametrize("split_k", [2, 3, 5])
@pytest.mark.parametrize("a_tri", [1, 2])
def test_triangular_split_k(launch, a_tri, split_k):
    """K slices of a triangular operand: the top row tiles (a_tri = 1) / bottom row tiles (a_tri = 2) own slices whose K
    range is empty.  Those come back as zeros, not as the NaN the slices were filled with."""
    for (layout, tile), m in itertools.product(TRI_KERNELS, (129, 257, 300)):
        bld = ArenaBuilder(m + split_k)
        r = bld.gemm(m, 64, m, layout, alpha=1.0, beta=1.0, a_tri=a_tri, pad_a=7, pad_c=5, split_k=split_k)
        arena, idx = bld.finish()
        what = (a_tri, split_k, layout, tile, m)
        out = launch(arena, idx, [r], m, 64, layout, tile, split_k=split_k, tri=1)
        exp, mask = check(out, arena, idx, [r], split_k, what=what)
        total = sum_slices(out, r, split_k)
        err = np.abs(total - sum_slices(exp, r, split_k)).max()
        assert err <= 4 * EPS * m * 2, (what, err)
        # rows of a slice that lies wholly in the excluded part of A: structural zeros
        chunk = split_chunk(m, split_k)
        i = np.arange(m)
        empty = 0
        for s in range(split_k):
            lo, hi = min(m, s * chunk), min(m, (s + 1) * chunk)
            rows = i[i < lo] if a_tri == 1 else i[i >= hi - 1]
            pos = int(r["c"]) + s * int(r["split_stride"]) + rows[:, None] + np.arange(64)[None, :] * int(r["ldc"])
            assert (out[pos] == 0.0).all(), (what, s)
            empty += rows.size
        assert empty > 0, what


# ---- gather lists -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_gather_one_record(launch, tile, beta):
    """A's and B's k axis through index lists into wider operands, C's columns scattered into a wider C; every list also
    absent.  Both gather instantiations (128 x 64, 64 x 64).  Equal to the plain launch on host-gathered operands."""
    rs = np.random.RandomState(tile)
    for (m, n), k, lists in itertools.product([(1, 1), (37, 100), (64, 64), (65, 129), (150, 300)],
                                              (0, 1, 15, 16, 17, 31, 33, 100), itertools.product((0, 1), repeat=3)):
        wide_a, wide_b, wide_c = k + 9, k + 5, n + 6
        ka = rs.permutation(wide_a)[:k] if lists[0] else np.arange(k)
        kb = rs.permutation(wide_b)[:k] if lists[1] else np.arange(k)
        jc = rs.permutation(wide_c)[:n] if lists[2] else np.arange(n)
        bld = ArenaBuilder(m + n + k)
        r = record(m=m, n=n, k=k, beta=beta, sa_i=1, sa_k=m + 3, sb_k=1, sb_j=wide_b + 1, ldc=m + 2)
        r["a"] = bld.matrix(m, wide_a, m + 3)
        r["b"] = bld.matrix(wide_b, n, wide_b + 1)
        r["c"] = bld.matrix(m, wide_c, m + 2, finite=beta != 0.0)
        for name, on, values in (("a_kidx", lists[0], ka), ("b_kidx", lists[1], kb), ("c_jidx", lists[2], jc)):
            if on:
                r[name] = bld.ints(values)
        arena, idx = bld.finish()
        what = (tile, beta, m, n, k, lists)
        out = launch(arena, idx, [r], m, n, AmBk, tile, gather=1)
        check(out, arena, idx, [r], what=what)
        # the plain launch on the gathered operands, packed
        pa, pb, pc = positions(r, idx)
        bld2 = ArenaBuilder(0)
        r2 = record(m=m, n=n, k=k, beta=beta, sa_i=1, sa_k=m, sb_k=1, sb_j=k, ldc=m)
        r2["a"] = bld2.block(arena[pa].T)
        r2["b"] = bld2.block(arena[pb].T)
        r2["c"] = bld2.block(arena[pc].T)
        arena2, idx2 = bld2.finish()
        out2 = launch(arena2, idx2, [r2], m, n, AmBk, tile)
        assert np.array_equal(out[pc], out2[positions(r2, idx2)[2]]), what


@pytest.mark.parametrize("tile", [10, 12, 13])
def test_gather_grouped_like_a_merge_level(launch, tile):
    """2 x nodes x batch records as the divide and conquer lays a level out: the two halves of a merge share B and the
    column list of C and differ in rows and K; sizes differ per node; n = 0, k = 0 and both occur (the device writes
    them).  Columns of the new eigenvector matrix that no record names keep their bits."""
    ntot, batch = 230, 2
    nodes = [(0, 70), (70, 101), (101, 165), (165, 166), (166, 230)]          # [lo, hi)
    rs = np.random.RandomState(tile)
    bld = ArenaBuilder(tile)
    recs = []
    for b in range(batch):
        q_old = bld.matrix(ntot, ntot, ntot + 1)
        u = bld.matrix(ntot, ntot, ntot + 2)
        q_new = bld.matrix(ntot, ntot, ntot + 1, finite=False)
        for g, (lo, hi) in enumerate(nodes):
            size = hi - lo
            mid = lo + (size + 1) // 2
            n = [size - 7, 0, size, 1, 0][g] if b == 0 else rs.randint(0, size + 1)
            c_jidx = bld.ints(lo + rs.permutation(size))
            for half, (r0, r1) in enumerate(((lo, mid), (mid, hi))):
                k = [rs.randint(1, size + 1), 5, 0 if half else size, half, 0][g] if b == 0 else rs.randint(0, size + 1)
                r = record(m=r1 - r0, n=n, k=k, sa_i=1, sa_k=ntot + 1, sb_k=1, sb_j=ntot + 2, ldc=ntot + 1)
                r["a"] = q_old + r0
                r["a_kidx"] = bld.ints(lo + rs.permutation(size)[:k])
                r["b"] = u + lo * (ntot + 2) + lo
                r["b_kidx"] = bld.ints(rs.permutation(size)[:k])
                r["c"] = q_new + r0
                r["c_jidx"] = c_jidx
                recs.append(r)
    arena, idx = bld.finish()
    max_n = max(hi - lo for lo, hi in nodes)
    out = launch(arena, idx, recs, (max_n + 1) // 2, max_n, AmBk, tile, gather=1)
    _, mask = check(out, arena, idx, recs, what=tile)
    assert mask.any()


# ---- grouped launches without lists -----------------------------------------------------------------------------------
GROUPS = [
    # max_m = 200 -> 4 row tiles of 64; 6 column tiles x 3 records = 18 groups, no multiple of the 8 XCDs
    [(200, 330, 70), (130, 64, 33), (1, 330, 16)],
    # max_m = 300 -> 3 row tiles of 128; 3 x 3 = 9 groups
    [(300, 150, 40), (129, 150, 17), (300, 1, 100)],
    [(64, 64, 0), (65, 63, 1), (17, 128, 129)],
]


@pytest.mark.parametrize("tile", [10, 11, 12, 13])
@pytest.mark.parametrize("layout", [AmBk, AkBk, AmBn])
@pytest.mark.parametrize("group", [0, 1, 2])
def test_plain_grouped_launch(launch, group, layout, tile):
    """Three records of different shapes under one max_m x max_n, operands and C as views with larger leading dimensions.
    Tile 13 on group 0 and tile 12 on group 1 run the launch that pairs the row tiles of a column panel on one XCD with a
    last round of groups that is not full."""
    bld = ArenaBuilder(group)
    recs = [bld.gemm(m, n, k, layout, alpha=(1.0, -1.0, 2.5)[t], beta=(0.0, 1.0, 1.0)[t], pad_a=3, pad_b=2, pad_c=4)
            for t, (m, n, k) in enumerate(GROUPS[group])]
    arena, idx = bld.finish()
    max_m, max_n = max(s[0] for s in GROUPS[group]), max(s[1] for s in GROUPS[group])
    out = launch(arena, idx, recs, max_m, max_n, layout, tile)
    check(out, arena, idx, recs, what=(group, layout, tile))


@pytest.mark.parametrize("lower_only", [1, 2])
@pytest.mark.parametrize("row_off,col_off", [(0, 0), (64, 0), (0, 64), (5, 70), (1, 65)])
def test_lower_only_with_offsets(launch, lower_only, row_off, col_off):
    """Only (row + row_off) >= (col + col_off) is stored (2: with row | 1): whole tiles are skipped, partial ones masked."""
    for m, tile, layout in itertools.product((70, 130), (10, 11, 12, 13), (AmBn, AmBk)):
        bld = ArenaBuilder(m)
        r = bld.gemm(m, m, 40, layout, alpha=-1.0, beta=1.0, lower_only=lower_only, row_off=row_off, col_off=col_off, pad_c=3)
        arena, idx = bld.finish()
        out = launch(arena, idx, [r], m, m, layout, tile)
        check(out, arena, idx, [r], what=(lower_only, row_off, col_off, m, tile, layout))


@pytest.mark.parametrize("lower_only", [1, 2])
@pytest.mark.parametrize("tile", [10, 11, 12, 13])
def test_lower_grid_of_three_records(launch, lower_only, tile):
    """The launch that only holds the tiles on and below the diagonal, for three square records of different orders."""
    bld = ArenaBuilder(tile)
    recs = [bld.gemm(m, m, 48, AmBn, alpha=-1.0, beta=1.0, lower_only=lower_only, pad_c=1) for m in (130, 200, 70)]
    arena, idx = bld.finish()
    out = launch(arena, idx, recs, 200, 200, AmBn, tile, lower_grid=1)
    _, mask = check(out, arena, idx, recs, what=(lower_only, tile))
    out0 = launch(arena, idx, recs, 200, 200, AmBn, tile, lower_grid=0)
    assert np.array_equal(out[mask], out0[mask])


# ---- record lists longer than one grid --------------------------------------------------------------------------------
@pytest.mark.parametrize("count,split_k", [(65536 + 7, 1), (40000, 2)])
def test_chunked_record_lists(launch, count, split_k):
    """More records x slices than grid.z holds: the list goes out in chunks.  4 x 4 x 3 records that share A and B, one C
    and one alpha each; every C is checked (K = 3: the second slice of a split record is empty and stored as zeros)."""
    m = n = 4
    k = 3
    bld = ArenaBuilder(count)
    a, b = bld.matrix(m, k), bld.matrix(k, n)
    c = bld.block(np.full(count * split_k * m * n, np.nan))
    arena, idx = bld.finish()
    recs = np.zeros(count, REC)
    recs["a_kidx"] = recs["b_kidx"] = recs["c_jidx"] = -1
    recs["m"], recs["n"], recs["k"] = m, n, k
    recs["a"], recs["sa_i"], recs["sa_k"] = a, 1, m
    recs["b"], recs["sb_k"], recs["sb_j"] = b, 1, k
    recs["c"] = c + np.arange(count, dtype=np.int64) * (split_k * m * n)
    recs["ldc"], recs["split_stride"] = m, m * n
    recs["alpha"] = 1.0 + 0.25 * (np.arange(count) % 5)
    recs["beta"] = 0.0
    out = launch(arena, idx, recs, m, n, AmBk, 10, split_k=split_k)
    # the model on the records around every chunk boundary, and all records by their closed form alpha_r A B
    per = 65535 // split_k
    near = np.unique(np.concatenate([np.arange(3), np.arange(count - 3, count)]
                                    + [np.arange(e - 3, e + 3) for e in range(per, count, per)]))
    exp, mask = gemm_records_reference(arena, idx, recs[near], split_k)
    assert np.isfinite(out[mask]).all() and np.abs(out[mask] - exp[mask]).max() <= 4 * EPS * k * 3.0
    untouched = np.ones(arena.size, bool)
    untouched[c:c + count * split_k * m * n] = False
    assert same_bits(out[untouched], arena[untouched]).all()
    got = out[c:c + count * split_k * m * n].reshape(count, split_k, n, m)
    p = (arena[a:a + m * k].reshape(k, m).T @ arena[b:b + k * n].reshape(n, k).T).T          # (n, m): column-major C
    want = recs["alpha"][:, None, None] * p[None]
    assert np.isfinite(got).all()
    err = np.abs(got[:, 0] - want).max(axis=(1, 2))
    assert (err <= 4 * EPS * k * (recs["alpha"] + 1)).all(), (int(err.argmax()), float(err.max()))
    assert (got[:, 1:] == 0.0).all()


# ---- what the entry refuses -------------------------------------------------------------------------------------------
def test_entry_refuses_records_that_point_outside(launch):
    """Nothing is launched on a record whose operands, strides or list entries reach outside the arenas, whose strides
    do not match the layout, or that asks for beta C alone (alpha == 0, beta != 0)."""
    bld = ArenaBuilder(0)
    good = bld.gemm(20, 30, 10, AmBk, beta=1.0, pad_c=2)
    lst = bld.ints(np.arange(30))
    far = bld.ints([0, 1, 2, 3, 4, 5, 6, 7, 8, 1 << 20])
    neg = bld.ints([0, 1, 2, 3, 4, -1, 6, 7, 8, 9])
    arena, idx = bld.finish()
    assert same_bits(launch(arena, idx, [good], 20, 30, AmBk, 13, gather=1), launch(arena, idx, [good], 20, 30, AmBk, 13)).all()

    def bad(gather=0, tri=0, layout=AmBk, split_k=1, lower_grid=0, max_m=20, max_n=30, **fields):
        r = good.copy()
        for name, value in fields.items():
            r[name] = value
        out = launch(arena, idx, [r], max_m, max_n, layout, 13, split_k=split_k, gather=gather, tri=tri,
                     lower_grid=lower_grid, expect=1)
        assert same_bits(out, arena).all()

    bad(a=arena.size - 20 * 10 + 1)
    bad(b=-1)
    bad(c=arena.size - 5)
    bad(ldc=19)
    bad(ldc=arena.size)
    bad(sa_k=arena.size)
    bad(sb_j=-3)
    bad(m=21)
    bad(n=31)
    bad(k=1 << 30)
    bad(sa_i=2)
    bad(layout=AkBk)
    bad(a_tri=1)
    bad(c_jidx=lst)
    bad(gather=1, c_jidx=idx.size - 29)
    bad(gather=1, a_kidx=idx.size - 9)        # ten entries from there run past the end of the int arena
    bad(gather=1, a_kidx=far)                 # an entry that leads outside the arena
    bad(gather=1, b_kidx=neg)
    bad(split_k=2, split_stride=arena.size)
    bad(lower_grid=1, layout=AmBn)
    bad(alpha=0.0)
    bad(alpha=np.nan)
    bad(lower_only=3)


def test_one_record_entry_refuses_alpha_zero():
    from springcraft_amd import _hip

    fn = _hip.lib().sc_dbg_gemm_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_double, C.c_double, C.c_int]
    z = np.ones(16)
    args = (_hip.context().handle, z.ctypes.data, z.ctypes.data, z.ctypes.data, 4, 4, 4, 0, 10, 1)
    assert fn(*args, 0.0, 1.0, 0) == 1
    assert fn(*args, 0.0, 0.0, 0) == 0 and (z == 0.0).all()
