"""
The record semantics of one grouped f64 GEMM launch (springcraft_amd/csrc/gemm_f64.h) restated in float64 NumPy, and a
builder for the arenas the record-level debug entry sc_dbg_gemm_records_host takes (include/springcraft_hip_debug.h).

A launch works on one arena of doubles and one arena of ints.  A record (REC, the NumPy mirror of sc_dbg_gemm_record)
holds element offsets into them:

    C(i, j) = beta C(i, j) + alpha sum_k A(i, k) B(k, j),    0 <= i < m, 0 <= j < n, 0 <= k < K
    A(i, k) = arena[a + i sa_i + ka(k) sa_k],   ka(k) = idx[a_kidx + k] or k        a_tri 1: counts for i >= k only
    B(k, j) = arena[b + kb(k) sb_k + j sb_j],   kb(k) = idx[b_kidx + k] or k        a_tri 2: counts for k > i only
    C(i, j) = arena[c + i + jc(j) ldc],         jc(j) = idx[c_jidx + j] or j
    lower_only 1: only (i + row_off) >= (j + col_off) is stored; 2: only ((i + row_off) | 1) >= (j + col_off)
    split_k > 1: beta is ignored and slice s stores alpha sum_{k in slice s} A B to c + s split_stride; a slice is
    ceil(K / split_k) rounded up to the kernel's K step of 16.

tests/test_gemm_records_host.py checks this model against dense products; tests/test_gemm_records_gpu.py checks the
kernels against the model.
"""
import numpy as np

AmBk, AkBk, AmBn = 0, 1, 2          # kGemmAmBk, kGemmAkBk, kGemmAmBn
K_STEP = 16

REC = np.dtype([(f, "<i8") for f in ("a", "b", "c", "a_kidx", "b_kidx", "c_jidx", "sa_i", "sa_k", "sb_k", "sb_j", "ldc",
                                     "split_stride")]
               + [("alpha", "<f8"), ("beta", "<f8")]
               + [(f, "<i4") for f in ("m", "n", "k", "lower_only", "row_off", "col_off", "a_tri", "reserved")])
assert REC.itemsize == 144


def record(**fields):
    """One record: no lists, alpha = 1, everything else 0 unless given."""
    r = np.zeros((), REC)
    r["a_kidx"] = r["b_kidx"] = r["c_jidx"] = -1
    r["alpha"] = 1.0
    for name, value in fields.items():
        r[name] = value
    return r


def records(recs):
    """The records of one launch as one contiguous array."""
    out = np.zeros(len(recs), REC)
    for t, r in enumerate(recs):
        out[t] = r
    return out


def split_chunk(k, split_k):
    """K entries per slice of a split-K launch."""
    per = -(-k // split_k)
    return -(-per // K_STEP) * K_STEP


def tri_keep(a_tri, m, k):
    """(m, k) mask of the entries of A that count."""
    i, kk = np.arange(m)[:, None], np.arange(k)[None, :]
    return i >= kk if a_tri == 1 else kk > i if a_tri == 2 else np.ones((m, k), bool)


def stored(r):
    """(m, n) mask of the entries of C the record stores."""
    i, j = np.arange(int(r["m"]))[:, None], np.arange(int(r["n"]))[None, :]
    lo = int(r["lower_only"])
    if lo == 0:
        return np.ones((i.size, j.size), bool)
    row = i + int(r["row_off"])
    return (row | 1 if lo == 2 else row) >= j + int(r["col_off"])


def positions(r, idx):
    """Arena positions of A (m, k), B (k, n) and C (m, n) of a record."""
    m, n, k = int(r["m"]), int(r["n"]), int(r["k"])
    i, j, kk = np.arange(m, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(k, dtype=np.int64)

    def through(off, plain):
        off = int(off)
        return plain if off < 0 else np.asarray(idx[off:off + plain.size], dtype=np.int64)

    ka, kb, jc = through(r["a_kidx"], kk), through(r["b_kidx"], kk), through(r["c_jidx"], j)
    pa = int(r["a"]) + i[:, None] * int(r["sa_i"]) + ka[None, :] * int(r["sa_k"])
    pb = int(r["b"]) + kb[:, None] * int(r["sb_k"]) + j[None, :] * int(r["sb_j"])
    pc = int(r["c"]) + i[:, None] + jc[None, :] * int(r["ldc"])
    return pa, pb, pc


def gemm_records_reference(arena, idx, recs, split_k=1, with_bound=False):
    """
    What one launch of `recs` leaves in `arena`: (expected arena, boolean mask of the entries the launch may write).
    Every record reads the arena as it was before the launch.  with_bound: also the per-entry error bound of the kernel
    tests, 4 eps max(K, 1) (|alpha| + |beta| + 1), 0 outside the mask.
    """
    arena = np.asarray(arena, dtype=np.float64)
    out = arena.copy()
    mask = np.zeros(arena.shape, bool)
    bound = np.zeros(arena.shape)
    eps = np.finfo(np.float64).eps
    for r in recs:
        m, n, k = int(r["m"]), int(r["n"]), int(r["k"])
        if m == 0 or n == 0:
            continue
        pa, pb, pc = positions(r, idx)
        a = arena[pa]
        if int(r["a_tri"]):
            a = np.where(tri_keep(int(r["a_tri"]), m, k), a, 0.0)
        b = arena[pb]
        st = stored(r)
        alpha, beta = float(r["alpha"]), float(r["beta"])
        tol = 4 * eps * max(k, 1) * (abs(alpha) + abs(beta) + 1)
        if split_k > 1:
            chunk = split_chunk(k, split_k)
            for s in range(split_k):
                lo, hi = min(k, s * chunk), min(k, (s + 1) * chunk)
                p = alpha * (a[:, lo:hi] @ b[lo:hi, :])
                pos = pc[st] + s * int(r["split_stride"])
                out[pos], mask[pos], bound[pos] = p[st], True, tol
        else:
            p = alpha * (a @ b)
            if beta != 0.0:
                p = p + beta * arena[pc]
            pos = pc[st]
            out[pos], mask[pos], bound[pos] = p[st], True, tol
    return (out, mask, bound) if with_bound else (out, mask)


def gemm_records_reads(arena_len, idx, recs, split_k=1):
    """Boolean mask of the arena entries the model reads for a launch."""
    reads = np.zeros(arena_len, bool)
    for r in recs:
        m, n, k = int(r["m"]), int(r["n"]), int(r["k"])
        if m == 0 or n == 0:
            continue
        pa, pb, pc = positions(r, idx)
        reads[pa[tri_keep(int(r["a_tri"]), m, k)]] = True
        reads[pb] = True
        if split_k <= 1 and float(r["beta"]) != 0.0:
            reads[pc] = True
    return reads


def same_bits(x, y):
    """Elementwise: the same bit pattern (NaN == NaN, +0 != -0)."""
    return np.ascontiguousarray(x).view(np.uint64) == np.ascontiguousarray(y).view(np.uint64)


class ArenaBuilder:
    """
    Lays operands out in one arena with gaps between them.  Everything a launch must not read is NaN: the gaps, the
    padding between a matrix's extent and its leading dimension, the part of A that a_tri excludes, and C where beta == 0
    (or the launch is split: the slices).  Operand entries are uniform in [-1, 1].
    """
    GAP = 19

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.parts, self.size = [], 0
        self.int_parts, self.int_size = [], 0

    def block(self, values):
        """A 1-D block behind a gap: its offset."""
        values = np.asarray(values, dtype=np.float64).ravel()
        self.parts += [np.full(self.GAP, np.nan), values]
        off = self.size + self.GAP
        self.size = off + values.size
        return off

    def matrix(self, nx, ny, ld=None, keep=None, finite=True):
        """nx x ny entries, (x, y) at offset + x + y ld; keep: (nx, ny) mask of the entries that are not NaN."""
        ld = nx if ld is None else ld
        assert ld >= nx
        v = np.full((ny, ld), np.nan)
        if finite:
            v[:, :nx] = self.rs.uniform(-1, 1, (ny, nx))
            if keep is not None:
                v[:, :nx][~np.asarray(keep).T] = np.nan
        return self.block(v)

    def ints(self, values):
        """An index list behind a short gap of zeros: its offset in the int arena."""
        values = np.asarray(values, dtype=np.int32).ravel()
        self.int_parts += [np.zeros(3, np.int32), values]
        off = self.int_size + 3
        self.int_size = off + values.size
        return off

    def gemm(self, m, n, k, layout, alpha=1.0, beta=0.0, a_tri=0, lower_only=0, row_off=0, col_off=0, pad_a=0, pad_b=0,
             pad_c=0, split_k=1, a=None, b=None):
        """A record without lists whose operands are views with leading dimensions extent + pad.  a / b: (offset, two
        strides) of an operand laid out earlier, to share it."""
        r = record(m=m, n=n, k=k, alpha=alpha, beta=beta, a_tri=a_tri, lower_only=lower_only, row_off=row_off,
                   col_off=col_off)
        keep = tri_keep(a_tri, m, k) if a_tri else None
        if a is None:
            if layout == AkBk:
                a = (self.matrix(k, m, k + pad_a, None if keep is None else keep.T), k + pad_a, 1)
            else:
                a = (self.matrix(m, k, m + pad_a, keep), 1, m + pad_a)
        if b is None:
            if layout == AmBn:
                b = (self.matrix(n, k, n + pad_b), n + pad_b, 1)
            else:
                b = (self.matrix(k, n, k + pad_b), 1, k + pad_b)
        r["a"], r["sa_i"], r["sa_k"] = a
        r["b"], r["sb_k"], r["sb_j"] = b
        r["ldc"] = m + pad_c
        if split_k > 1:
            r["split_stride"] = (m + pad_c) * n + 11
            r["c"] = self.block(np.full(split_k * int(r["split_stride"]), np.nan))
        else:
            r["c"] = self.matrix(m, n, m + pad_c, finite=beta != 0.0)
        return r

    def finish(self):
        """(arena, int arena); the arena ends with a gap."""
        arena = np.concatenate(self.parts + [np.full(self.GAP, np.nan)])
        idx = np.concatenate(self.int_parts + [np.zeros(3, np.int32)])
        return arena, idx


def sum_slices(arena, r, split_k):
    """(m, n) sum of the K slices of a split record (column-major positions of an unscattered C)."""
    m, n, ldc = int(r["m"]), int(r["n"]), int(r["ldc"])
    pos = int(r["c"]) + np.arange(m)[:, None] + np.arange(n)[None, :] * ldc
    return sum(arena[pos + s * int(r["split_stride"])] for s in range(split_k))
