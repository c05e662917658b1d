"""
The NumPy model of a grouped GEMM launch (tests/gemm_records.py) against dense products written out by hand, and the arena
builder's promises.  No GPU: what tests/test_gemm_records_gpu.py compares the kernels with has to be right on its own.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

from tests.gemm_records import (AkBk, AmBk, AmBn, REC, ArenaBuilder, gemm_records_reads, gemm_records_reference, record,
                                records, same_bits, split_chunk, sum_slices)

ROOT = dirname(dirname(__file__))


def dense(arena, off, rows, cols, s_row, s_col):
    """The (rows, cols) matrix at `off` with the two strides, by plain loops."""
    out = np.empty((rows, cols))
    for i in range(rows):
        for j in range(cols):
            out[i, j] = arena[off + i * s_row + j * s_col]
    return out


def test_record_type_mirrors_the_header():
    text = open(join(ROOT, "include", "springcraft_hip_debug.h")).read()
    body = re.search(r"typedef struct sc_dbg_gemm_record \{(.*?)\} sc_dbg_gemm_record;", text, re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(long long|double|int)\s+([a-z_, ]+);", body):
        kind = {"long long": "<i8", "double": "<f8", "int": "<i4"}[ctype]
        fields += [(name.strip(), kind) for name in names.split(",")]
    assert fields == [(name, REC[name].str) for name in REC.names]
    assert [REC.fields[name][1] for name in REC.names] == list(np.cumsum([0] + [REC[name].itemsize for name in REC.names])[:-1])


@pytest.mark.parametrize("layout", [AmBk, AkBk])
@pytest.mark.parametrize("a_tri", [1, 2])
@pytest.mark.parametrize("m,k", [(1, 1), (17, 17), (40, 23), (23, 40)])
def test_tri_record_is_the_dense_product_of_the_masked_operand(layout, a_tri, m, k):
    n = 9
    bld = ArenaBuilder(m + k)
    r = bld.gemm(m, n, k, layout, alpha=-1.5, beta=1.0, a_tri=a_tri, pad_a=7, pad_b=2, pad_c=5)
    arena, idx = bld.finish()
    a = dense(arena, int(r["a"]), m, k, int(r["sa_i"]), int(r["sa_k"]))
    for i in range(m):
        for kk in range(k):
            counts = i >= kk if a_tri == 1 else kk > i
            assert np.isnan(a[i, kk]) != counts          # the builder poisons exactly the excluded part
            if not counts:
                a[i, kk] = 0.0
    b = dense(arena, int(r["b"]), k, n, int(r["sb_k"]), int(r["sb_j"]))
    c0 = dense(arena, int(r["c"]), m, n, 1, int(r["ldc"]))
    out, mask = gemm_records_reference(arena, idx, [r])
    got = dense(out, int(r["c"]), m, n, 1, int(r["ldc"]))
    assert np.allclose(got, c0 - 1.5 * (a @ b), rtol=0, atol=1e-13)
    assert mask.sum() == m * n and same_bits(out[~mask], arena[~mask]).all()


@pytest.mark.parametrize("lists", [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)])
@pytest.mark.parametrize("k", [0, 1, 17])
def test_gather_record_is_the_dense_product_of_the_gathered_operands(lists, k):
    m, n, wide_a, wide_b, wide_c = 11, 7, 30, 25, 12
    bld = ArenaBuilder(k)
    rs = np.random.RandomState(5)
    ka, kb, jc = rs.permutation(wide_a)[:k], rs.permutation(wide_b)[:k], rs.permutation(wide_c)[:n]
    r = record(m=m, n=n, k=k, beta=1.0, alpha=2.0, sa_i=1, sa_k=m + 3, sb_k=1, sb_j=wide_b + 1, ldc=m + 2)
    r["a"] = bld.matrix(m, wide_a, m + 3)
    r["b"] = bld.matrix(wide_b, n, wide_b + 1)
    r["c"] = bld.matrix(m, wide_c, m + 2)
    if lists[0]:
        r["a_kidx"] = bld.ints(ka)
    if lists[1]:
        r["b_kidx"] = bld.ints(kb)
    if lists[2]:
        r["c_jidx"] = bld.ints(jc)
    arena, idx = bld.finish()
    a = dense(arena, int(r["a"]), m, wide_a, 1, m + 3)[:, ka if lists[0] else np.arange(k)]
    b = dense(arena, int(r["b"]), wide_b, n, 1, wide_b + 1)[kb if lists[1] else np.arange(k), :]
    c0 = dense(arena, int(r["c"]), m, wide_c, 1, m + 2)
    cols = jc if lists[2] else np.arange(n)
    want = c0.copy()
    want[:, cols] = c0[:, cols] + 2.0 * (a @ b)
    out, mask = gemm_records_reference(arena, idx, [r])
    assert np.allclose(dense(out, int(r["c"]), m, wide_c, 1, m + 2), want, rtol=0, atol=1e-13)
    written = dense(mask.astype(float), int(r["c"]), m, wide_c, 1, m + 2) != 0
    assert written[:, cols].all() and written.sum() == m * n == mask.sum()
    assert same_bits(out[~mask], arena[~mask]).all()


@pytest.mark.parametrize("lower_only", [1, 2])
@pytest.mark.parametrize("row_off,col_off", [(0, 0), (64, 0), (0, 64), (5, 70), (1, 65)])
def test_lower_only_record_leaves_the_complement_untouched(lower_only, row_off, col_off):
    m = n = 75
    bld = ArenaBuilder(3)
    r = bld.gemm(m, n, 4, AmBn, beta=1.0, lower_only=lower_only, row_off=row_off, col_off=col_off, pad_c=3)
    arena, idx = bld.finish()
    out, mask = gemm_records_reference(arena, idx, [r])
    full, _ = gemm_records_reference(arena, idx, [bld_copy(r, lower_only=0)])
    for i in range(m):
        for j in range(n):
            row = i + row_off
            keep = (row | 1 if lower_only == 2 else row) >= j + col_off
            p = int(r["c"]) + i + j * int(r["ldc"])
            assert mask[p] == keep
            assert out[p] == (full[p] if keep else arena[p])
    assert same_bits(out[~mask], arena[~mask]).all()


def bld_copy(r, **fields):
    c = r.copy()
    for name, value in fields.items():
        c[name] = value
    return c


@pytest.mark.parametrize("k,split_k", [(0, 2), (15, 2), (33, 3), (100, 5), (129, 3)])
def test_split_slices_add_up_and_tile_k_in_steps(k, split_k):
    m, n = 6, 5
    bld = ArenaBuilder(k)
    r = bld.gemm(m, n, k, AkBk, alpha=0.5, beta=3.0, pad_a=1, pad_c=2, split_k=split_k)
    arena, idx = bld.finish()
    out, mask = gemm_records_reference(arena, idx, [r], split_k)
    a = dense(arena, int(r["a"]), m, k, int(r["sa_i"]), int(r["sa_k"]))
    b = dense(arena, int(r["b"]), k, n, int(r["sb_k"]), int(r["sb_j"]))
    assert np.allclose(sum_slices(out, r, split_k), 0.5 * (a @ b), rtol=0, atol=1e-13)       # beta is ignored
    assert mask.sum() == split_k * m * n and np.isfinite(out[mask]).all()
    chunk = split_chunk(k, split_k)
    assert chunk % 16 == 0 and chunk * split_k >= k and (chunk - 16) * split_k < max(k, 1)
    for s in range(split_k):
        if s * chunk >= k:                                # an empty slice is stored as zeros
            pos = int(r["c"]) + s * int(r["split_stride"]) + np.arange(m)
            assert (out[pos] == 0.0).all()


def test_records_of_one_launch_read_the_arena_as_it_was():
    bld = ArenaBuilder(9)
    r0 = bld.gemm(5, 4, 3, AmBk, beta=1.0, pad_c=1)
    # the second record reads the first one's C as its B: it sees the values from before the launch
    r1 = bld.gemm(6, 4, 5, AmBn, b=(int(r0["c"]), 1, int(r0["ldc"])))
    r2 = bld.gemm(0, 4, 5, AmBk)
    r3 = bld.gemm(4, 0, 5, AmBk)
    arena, idx = bld.finish()
    both, mask = gemm_records_reference(arena, idx, records([r0, r1, r2, r3]))
    one, mask1 = gemm_records_reference(arena, idx, [r1])
    assert same_bits(both[mask1], one[mask1]).all()
    assert mask.sum() == 5 * 4 + 6 * 4


def test_builder_poisons_nothing_the_model_reads():
    bld = ArenaBuilder(1)
    recs = [bld.gemm(33, 20, 33, AmBk, a_tri=1, beta=1.0, pad_a=7, pad_c=5),
            bld.gemm(20, 10, 31, AkBk, a_tri=2, pad_a=7, pad_b=3, pad_c=5),
            bld.gemm(12, 9, 40, AmBn, beta=-1.0, lower_only=2, pad_b=2),
            bld.gemm(12, 9, 40, AkBk, beta=1.0, split_k=3)]
    arena, idx = bld.finish()
    for split_k, part in ((1, recs[:3]), (3, recs[3:])):
        reads = gemm_records_reads(arena.size, idx, part, split_k)
        assert reads.any() and np.isfinite(arena[reads]).all()
        out, mask, bound = gemm_records_reference(arena, idx, part, split_k, with_bound=True)
        assert np.isfinite(out[mask]).all() and (bound[mask] > 0).all() and (bound[~mask] == 0).all()
    # and everything else is poisoned: gaps, padding, the excluded triangle, C with beta == 0, the slices
    reads = gemm_records_reads(arena.size, idx, recs[:3]) | gemm_records_reads(arena.size, idx, recs[3:], 3)
    assert np.isnan(arena[~reads]).all()
    assert np.isnan(arena[:ArenaBuilder.GAP]).all() and np.isnan(arena[-ArenaBuilder.GAP:]).all()
