"""
CPU-only checks for the batch consumers: the pure mapping from the reference's ``mode_subset`` (global ascending mode
indices, nma.py:161-168) to rows of a batch solver's ``w`` / ``v``, and the C ABI of the new entry points.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

ROOT = dirname(dirname(__file__))


@pytest.fixture(scope="module")
def rows():
    from springcraft_amd.batch import batch_mode_rows

    return batch_mode_rows


def test_full_spectrum_solver_rows_are_mode_indices(rows):
    assert np.array_equal(rows(None, 6, None, 30), np.arange(6, 30))
    assert np.array_equal(rows(None, 1, None, 30), np.arange(1, 30))
    assert np.array_equal(rows(np.arange(6, 16), 6, None, 30), np.arange(6, 16))
    got = rows([9, 7, 29, 9], 6, None, 30)
    assert np.array_equal(got, [9, 7, 29, 9]) and got.dtype == np.int32      # unsorted, repeated: kept as listed
    assert len(rows([], 6, None, 30)) == 0


def test_subset_by_index_solver_rows_are_offsets_from_lo(rows):
    assert np.array_equal(rows(None, 6, (0, 25), 300), np.arange(6, 26))     # the trivial modes it solved are skipped
    assert np.array_equal(rows(None, 6, (6, 25), 300), np.arange(0, 20))
    assert np.array_equal(rows(None, 6, (10, 25), 300), np.arange(0, 16))
    assert np.array_equal(rows(None, 1, (0, 9), 50), np.arange(1, 10))
    assert len(rows(None, 6, (0, 5), 300)) == 0                              # only trivial modes were solved
    assert len(rows(None, 6, (2, 4), 300)) == 0
    assert np.array_equal(rows([25, 6, 6], 6, (6, 25), 300), [19, 0, 0])
    assert np.array_equal(rows([25, 6, 6], 6, (0, 25), 300), [25, 6, 6])
    assert np.array_equal(rows(np.arange(1, 5), 1, (1, 9), 50), np.arange(0, 4))


@pytest.mark.parametrize("subset,solver,m", [([7, 26], (0, 25), 300), ([26], (6, 25), 300), ([7, 30], None, 30),
                                             ([6, 7, 8], (7, 25), 300), ([299], (6, 25), 300)])
def test_an_index_that_was_not_solved_names_the_solved_range(rows, subset, solver, m):
    lo, hi = solver if solver is not None else (0, m - 1)
    with pytest.raises(ValueError, match=f"holds modes {lo}\\.\\.{hi}"):
        rows(subset, 6, solver, m)


@pytest.mark.parametrize("subset,ntriv,solver", [([5, 7], 6, None), (np.arange(0, 10), 6, (0, 25)), ([0], 1, None),
                                                 ([3], 6, (6, 25)), ([-1], 6, None), ([-1], 1, (0, 9))])
def test_trivial_modes_raise_the_references_error(rows, subset, ntriv, solver):
    with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
        rows(subset, ntriv, solver, 300)


def test_a_window_takes_no_mode_subset(rows):
    assert rows(None, 6, None, 300, window=(1e-3, 2.0)) is None
    with pytest.raises(ValueError, match="subset_by_value"):
        rows([7, 8], 6, None, 300, window=(1e-3, 2.0))
    with pytest.raises(ValueError, match="subset_by_value"):
        rows([], 6, None, 300, window=(-np.inf, 2.0))


def test_non_integer_indices_are_rejected(rows):
    with pytest.raises(IndexError):
        rows([6.5, 7.0], 6, None, 300)


@pytest.mark.parametrize("ntriv", [6, 1])
@pytest.mark.parametrize("subset", [None, (0, 11), (6, 25), (9, 30), (0, 3)])
def test_from_row_start_is_the_first_non_trivial_row(rows, ntriv, subset):
    """
    "Every solved non-trivial mode" is SC_SEL_FROM_ROW from the number of trivial rows at the head of ``w`` / ``v``, one
    formula for both batch solvers: the first row ``batch_mode_rows(None, ...)`` lists, or ``nvec`` when it lists none.
    """
    from springcraft_amd.batch import _trivial_rows

    m = 33
    lo, hi = (0, m - 1) if subset is None else subset
    nvec = hi - lo + 1
    listed = rows(None, ntriv, subset, m)
    start = _trivial_rows(ntriv, lo, nvec)
    assert start == (int(listed[0]) if len(listed) else nvec)
    assert np.array_equal(listed, np.arange(start, nvec))
    assert start == sum(1 for r in range(nvec) if lo + r < ntriv)


def test_new_symbols_are_declared_exported_and_typed():
    from springcraft_amd import _hip

    names = ["sc_dev_modes_msf_f64", "sc_dev_modes_dcc_f64", "sc_dev_modes_workspace_bytes"]
    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    L = _hip.lib()
    for name in names:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "typedef struct sc_mode_selection" in header
    for const in ("SC_SEL_FROM_ROW", "SC_SEL_ROWS", "SC_SEL_PINV"):
        value = int(re.search(rf"#define {const} (\d+)", header).group(1))
        assert getattr(_hip, const) == value
    # the ctypes mirror of sc_mode_selection: kind, reserved, row0, d_rows, n_rows, rcond on 64-bit pointers
    import ctypes as C

    assert C.sizeof(_hip.ModeSelection) == 40
    assert [f[0] for f in _hip.ModeSelection._fields_] == ["kind", "reserved", "row0", "d_rows", "n_rows", "rcond"]


def test_workspace_query_follows_the_budget_not_the_batch():
    """
    The packed operands of dcc stay under the budget whatever the batch; what grows with the batch are the weights and the
    diagonals.  At the benchmarked shape (m = 6000, 64 structures) one structure's operands are 576 MB: one per launch.
    """
    from springcraft_amd import _hip

    L = _hip.lib()
    q = L.sc_dev_modes_workspace_bytes
    m = 6000
    one, many = q(m, m, 1, 3, m, 1, 0), q(m, m, 64, 3, m, 1, 0)
    pack = 2 * m * m * 8
    assert pack <= one <= pack + (1 << 20)
    assert many - one <= 64 * (m * 8 + 2000 * 8) + (1 << 16)
    # a budget below one structure's operands: chunks of floor(budget / (2 m 8)) rows
    small = q(m, m, 64, 3, m, 1, 64 << 20)
    assert small <= (64 << 20) + 64 * (m * 8 + 2000 * 8) + (1 << 16)
    # a 20-row list: all 64 structures in one launch
    assert q(m, 20, 64, 3, 20, 1, 0) >= 64 * 2 * 20 * m * 8
    # msf: partial sums of 48 chunks per structure, 1.6 % of the eigenvectors
    msf = q(m, m, 64, 3, m - 6, 0, 0)
    assert 64 * 48 * m * 8 <= msf <= 64 * 49 * m * 8 + 64 * m * 8 + (1 << 16)
    assert q(0, 0, 0, 3, 0, 0, 0) == 0 and q(m, m, 1, 2, m, 1, 0) == 0
