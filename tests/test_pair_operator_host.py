"""
Host side of the pair-list operator (springcraft_amd/pair_operator.py): the row starts, the symmetry check, the spring
rows and the argument checks that need no device.  NumPy only.
"""
import numpy as np
import pytest

from springcraft_amd import pair_operator as po


def directed(n, edges):
    """Both directions of ``edges``, sorted by first then second atom."""
    e = np.array(edges, dtype=np.int64).reshape(-1, 2)
    p = np.concatenate([e, e[:, ::-1]])
    return p[np.lexsort((p[:, 1], p[:, 0]))]


# empty rows at the start (atoms 0, 1), in the middle (4, 5) and at the end (9, 10)
GAPPY = directed(11, [(2, 3), (2, 6), (3, 7), (6, 8), (7, 8), (2, 8)])


def test_package_imports_without_a_gpu():
    import springcraft_amd as sc

    assert sc.PairOperator is po.PairOperator
    for name in ("deformation_energy", "spring_strain"):
        assert callable(getattr(sc.nma, name)) and name in sc.nma.__all__
        assert callable(getattr(sc.ANM, name)) and callable(getattr(sc.GNM, name))
    for name in ("operator", "residuals", "deformation_energy", "spring_strain"):
        assert hasattr(sc.RTB, name)


@pytest.mark.parametrize("pairs, n", [(GAPPY, 11), (GAPPY, 40), (directed(3, [(0, 1), (1, 2), (0, 2)]), 3),
                                      (np.empty((0, 2), dtype=np.int64), 1), (np.empty((0, 2), dtype=np.int64), 5)])
def test_row_start_is_searchsorted(pairs, n):
    start = po.pair_row_start(pairs, n)
    assert start.dtype == np.int64 and start.shape == (n + 1,)
    assert np.array_equal(start, np.searchsorted(pairs[:, 0], np.arange(n + 1)))
    assert start[0] == 0 and start[-1] == len(pairs)
    for i in range(n):
        assert np.all(pairs[start[i]: start[i + 1], 0] == i)


def test_row_start_gaps():
    start = po.pair_row_start(GAPPY, 11)
    count = np.diff(start)
    assert list(np.nonzero(count == 0)[0]) == [0, 1, 4, 5, 9, 10]
    assert count.sum() == len(GAPPY)


def test_row_start_rejects_bad_lists():
    with pytest.raises(ValueError, match="sorted"):
        po.pair_row_start(GAPPY[::-1], 11)
    with pytest.raises(ValueError, match="outside"):
        po.pair_row_start(GAPPY, 8)
    with pytest.raises(ValueError, match="outside"):
        po.pair_row_start(np.array([[-1, 2]]), 4)
    with pytest.raises(ValueError, match="shape"):
        po.pair_row_start(np.zeros((4, 3), dtype=np.int64), 4)
    with pytest.raises(ValueError, match="integer"):
        po.pair_row_start(np.zeros((4, 2)), 4)
    with pytest.raises(ValueError, match="positive"):
        po.pair_row_start(np.empty((0, 2), dtype=np.int64), 0)


def symmetric_gamma(pairs, seed=0):
    g = np.random.RandomState(seed).uniform(0.5, 2.0, (pairs.max() + 1, pairs.max() + 1))
    g = g + g.T
    return g[pairs[:, 0], pairs[:, 1]]


def test_symmetry_check_accepts_symmetric_constants():
    po.check_symmetric(GAPPY, symmetric_gamma(GAPPY), 11)
    po.check_symmetric(np.empty((0, 2), dtype=np.int64), np.empty(0), 3)
    g = symmetric_gamma(GAPPY)
    g[(GAPPY == [2, 3]).all(1) | (GAPPY == [3, 2]).all(1)] = np.nan   # (NaN both ways is symmetric)
    po.check_symmetric(GAPPY, g, 11)


@pytest.mark.parametrize("row", range(len(GAPPY)))
def test_symmetry_check_raises_on_one_flipped_entry(row):
    g = symmetric_gamma(GAPPY)
    g[row] = np.nextafter(g[row], np.inf)
    with pytest.raises(ValueError, match="asymmetric"):
        po.check_symmetric(GAPPY, g, 11)


def test_symmetry_check_rejects_broken_lists():
    g = symmetric_gamma(GAPPY)
    with pytest.raises(ValueError, match="reverse"):
        po.check_symmetric(GAPPY[1:], g[1:], 11)
    with pytest.raises(ValueError, match="sorted"):
        po.check_symmetric(GAPPY[::-1], g[::-1], 11)
    with pytest.raises(ValueError, match="sorted"):
        po.check_symmetric(np.concatenate([GAPPY[:1], GAPPY]), np.concatenate([g[:1], g]), 11)
    with pytest.raises(ValueError, match="itself"):
        po.check_symmetric(np.array([[1, 1]]), np.ones(1), 3)
    with pytest.raises(ValueError, match="force constants"):
        po.check_symmetric(GAPPY, g[:-1], 11)


def test_undirected_rows():
    idx = po.undirected(GAPPY)
    assert idx.dtype == np.int64
    assert np.array_equal(idx, [r for r, (i, j) in enumerate(GAPPY) if i < j])
    assert len(idx) * 2 == len(GAPPY)
    assert sorted(map(tuple, GAPPY[idx])) == sorted([(2, 3), (2, 6), (3, 7), (6, 8), (7, 8), (2, 8)])
    assert len(po.undirected(np.empty((0, 2), dtype=np.int64))) == 0
    with pytest.raises(ValueError, match="shape"):
        po.undirected(np.zeros(4, dtype=np.int64))


@pytest.mark.parametrize("dim", [0, 2, 4, "3", None, 3.5])
def test_dim_must_be_1_or_3(dim):
    with pytest.raises(ValueError, match="dim must be"):
        po._checked_dim(dim)
    # the constructors check it before they touch a device
    with pytest.raises(ValueError, match="dim must be"):
        po.PairOperator(np.zeros((3, 3)), None, dim=dim)
    with pytest.raises(ValueError, match="dim must be"):
        po.PairOperator.from_pairs(np.zeros((3, 3)), GAPPY, np.ones(len(GAPPY)), dim=dim)


def test_masses_as_for_a_model():
    coord = np.zeros((3, 3))
    assert po._model_masses(coord, None, 3) is None and po._model_masses(coord, False, 3) is None
    assert np.array_equal(po._model_masses(coord, [1, 2, 3], 3), [1.0, 2.0, 3.0])
    with pytest.raises(IndexError):
        po._model_masses(coord, [1, 2], 3)
    with pytest.raises(ValueError, match="must not be 0"):
        po._model_masses(coord, [1, 0, 3], 3)
    with pytest.raises(TypeError, match="AtomArray"):
        po._model_masses(coord, True, 3)
