"""
What tests/test_frame_neighbours_host.py and tests/test_frame_neighbours_gpu.py share: the NumPy specification of the frames'
neighbour bits (csrc/rmsd_matrix.hip's second epilogue, ``Ensemble.neighbours``) and the epilogue's tile / lane -> word map as
index arithmetic.

Specification.  ``d = rmsd_matrix_model.rmsd_matrix(frames, None, weights, fit, squared)``.  Frame f is valid when ``d[f, f]``
is not NaN (its G is finite).  ``near[f, g] = (d[f, g] <= cutoff or f == g) and valid[f] and valid[g]``: a valid frame is its
own neighbour, an invalid frame's row and column are empty.  ``bits`` (M, ceil(M / 64)) uint64: bit ``g & 63`` of word
``g >> 6`` of row f is ``near[f, g]``, the bits of the columns >= M are 0.  ``counts[f]`` is the row's popcount.  These are
the semantics of ``cluster_model.gromos``' ``near`` matrix, so its rounds on ``d`` are the rounds on the bits.

The map.  A workgroup of 512 threads owns the tile (tf, tg), tf >= tg, of 64 x 64 pairs: rows f = 64 tf + i, columns
g = 64 tg + c.  Thread tid: wavefront w = tid >> 6, fr = tid & 15, fk = (tid >> 4) & 3, fb = w & 3, gb0 = 2 (w >> 2).  Its
slot (j, r), j < 2, r < 4, is the pair i = 16 fb + 4 r + fk, c = 16 (gb0 + j) + fr.  The wavefront's ballot of slot (j, r) has
the thread's predicate at bit ``tid & 63`` = 16 fk + fr; lane 16 fk stores bits 16 fk .. 16 fk + 15 as quarter gb0 + j (a
uint16) of word i of the tile.  Then word i of the tile is word tg of row 64 tf + i; off the diagonal the transposed word of
column c -- bit i from word i of the tile -- is word tf of row 64 tg + c; a diagonal tile holds the pairs i > c only and is
ORed with its transpose and the diagonal.
"""
import numpy as np

from tests import rmsd_matrix_model as rm

TILE = 64
THREADS = 512


# ---- the specification ------------------------------------------------------------------------------------------------------------
def words_of(n):
    return (n + 63) // 64


def pack(near):
    """(M, words) uint64 of an (M, M) bool matrix, bit g & 63 of word g >> 6; the pad bits 0."""
    near = np.asarray(near, dtype=bool)
    n = near.shape[0]
    padded = np.zeros((n, 64 * words_of(near.shape[1])), dtype=np.uint64)
    padded[:, : near.shape[1]] = near
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(n, -1, 64) * weights[None, None, :]).sum(axis=2, dtype=np.uint64)


def unpack(bits, n):
    """(rows, n) bool of (rows, words) uint64 (or int64) words."""
    b = np.ascontiguousarray(bits).view(np.uint64)
    out = (b[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return out.reshape(b.shape[0], -1)[:, :n].astype(bool)


def popcounts(bits):
    """(rows,) int32: set bits per row, the pad bits included."""
    b = np.ascontiguousarray(bits).view(np.uint64)
    return unpack(b, 64 * b.shape[1]).sum(axis=1).astype(np.int32)


def near_of_matrix(dist, cutoff):
    """``(near (M, M) bool, valid (M,) bool)`` of a matrix with NaN rows and columns for its invalid items."""
    dist = np.asarray(dist, dtype=np.float64)
    valid = ~np.isnan(np.diag(dist))
    with np.errstate(invalid="ignore"):
        near = (dist <= cutoff) | np.eye(len(dist), dtype=bool)
    return near & valid[:, None] & valid[None, :], valid


def neighbours(frames, cutoff, weights=None, fit=True, squared=False):
    """``(bits (M, words) uint64, counts (M,) int32, valid (words,) uint64, dist)`` of the specification."""
    dist = rm.rmsd_matrix(frames, None, weights, fit, squared)
    near, valid = near_of_matrix(dist, cutoff)
    return pack(near), near.sum(axis=1).astype(np.int32), pack(valid[None, :])[0], dist


# ---- the epilogue's map -------------------------------------------------------------------------------------------------------------
def tiles(n):
    """The tiles (tf, tg), tf >= tg, in workgroup order."""
    t = (n + TILE - 1) // TILE
    return [(tf, tg) for tf in range(t) for tg in range(tf + 1)]


def slots(tid):
    """The eight ``(j, r, i, c)`` of thread ``tid``: its accumulator slot and the tile-local pair it holds."""
    w, fr, fk = tid >> 6, tid & 15, (tid >> 4) & 3
    fb, gb0 = w & 3, 2 * (w >> 2)
    return [(j, r, 16 * fb + 4 * r + fk, 16 * (gb0 + j) + fr) for j in range(2) for r in range(4)]


def ballot_store(tid, j, r):
    """``(word, quarter, bit, storing thread)``: where in the tile the predicate of slot (j, r) of thread ``tid`` lands."""
    w, lane = tid >> 6, tid & 63
    fk = lane >> 4
    fb, gb0 = w & 3, 2 * (w >> 2)
    return 16 * fb + 4 * r + fk, gb0 + j, lane - 16 * fk, (tid & ~63) | (16 * fk)


def tile_bits(tf, tg, n):
    """
    Every bit the workgroup of tile (tf, tg) gives to the bit matrix of n frames, as ``(row, word, bit, f, g)``: bit ``bit``
    of word ``word`` of row ``row`` is the predicate of the pair (f, g), f >= g.  Rows >= n are not stored; a column >= n
    gives a bit that is always 0 and is listed with the others.
    """
    diag = tf == tg
    out = []
    held = {}          # (word of the tile, bit) -> (f, g), through the ballots and the uint16 stores
    for tid in range(THREADS):
        for j, r, i, c in slots(tid):
            word, quarter, bit, _ = ballot_store(tid, j, r)
            key = (word, 16 * quarter + bit)
            assert key not in held
            held[key] = (TILE * tf + i, TILE * tg + c)
    for i in range(TILE):           # lanes 0..63: the rows' words; 64..127: the transposed words
        for c in range(TILE):
            f, g = held[(i, c)]
            if diag:
                if c < i:
                    out.append((f, tf, c, f, g))
                    out.append((g, tf, i, f, g))
                elif c == i:
                    out.append((f, tf, i, f, f))
            else:
                out.append((f, tg, c, f, g))
                out.append((g, tf, i, f, g))
    return [t for t in out if t[0] < n]
