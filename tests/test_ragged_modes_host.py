"""
Host-side logic of the ragged partial-spectrum solves and their consumers: ``ragged_subset_plan`` (what a
``RaggedBatchSolver`` may solve per padded slot), ``batch_mode_rows`` with the order of the smallest structure, and
``solve_ragged(..., subset_by_index=...)`` over gloo with the device solver replaced by the oracle.  No GPU and no
compiled library is needed.
"""
import os
import socket

import numpy as np
import pytest

from springcraft_amd.batch import batch_mode_rows, ragged_subset_plan, solve_ragged


# ---- 1. ragged_subset_plan ---------------------------------------------------------------------------------------------------
def test_plan_is_exported():
    import springcraft_amd.batch as batch

    assert "ragged_subset_plan" in batch.__all__


@pytest.mark.parametrize("dim", [1, 3])
def test_plan_full_spectrum(dim):
    sizes = [43, 50, 37, 64]
    p = ragged_subset_plan(sizes, dim)
    assert p["subset"] is None and p["window"] is None and p["max_modes"] is None
    assert p["nvec"] is None and p["first_row"] == 0
    assert p["row_limits"] == [dim * n for n in sizes]


@pytest.mark.parametrize("dim", [1, 3])
def test_plan_index_range(dim):
    sizes = [43, 50, 37, 64]
    top = dim * 37 - 1
    for lo, hi in ((0, 11), (6, 25), (top, top), (0, top)):
        p = ragged_subset_plan(sizes, dim, subset_by_index=(lo, hi))
        assert p["subset"] == (lo, hi) and p["window"] is None
        assert p["nvec"] == hi - lo + 1 and p["first_row"] == lo
        assert p["row_limits"] == [hi - lo + 1] * 4


@pytest.mark.parametrize("dim", [1, 3])
def test_plan_window(dim):
    sizes = [20, 64]
    for k in (1, 7, dim * 20):
        p = ragged_subset_plan(sizes, dim, subset_by_value=(0.5, np.inf), max_modes=k)
        assert p["window"] == (0.5, np.inf) and p["subset"] is None
        assert p["max_modes"] == k and p["nvec"] == k and p["first_row"] == 0
        assert p["row_limits"] == [k, k]


@pytest.mark.parametrize("dim", [1, 3])
def test_plan_rejects_what_the_smallest_structure_does_not_have(dim):
    sizes = [43, 50, 37, 64]
    with pytest.raises(ValueError, match=r"smallest structure \(2: 37 atoms\)"):
        ragged_subset_plan(sizes, dim, subset_by_index=(0, dim * 37))
    with pytest.raises(ValueError, match="smallest structure"):
        ragged_subset_plan(sizes, dim, subset_by_index=(5, 4))
    with pytest.raises(ValueError, match="smallest structure"):
        ragged_subset_plan(sizes, dim, subset_by_index=(-1, 4))
    with pytest.raises(ValueError, match=r"max_modes .* smallest structure \(2: 37 atoms\)"):
        ragged_subset_plan(sizes, dim, subset_by_value=(0.0, 1.0), max_modes=dim * 37 + 1)
    with pytest.raises(ValueError, match="max_modes"):
        ragged_subset_plan(sizes, dim, subset_by_value=(0.0, 1.0), max_modes=0)


def test_plan_keeps_the_rules_of_the_uniform_solver():
    sizes = [10, 12]
    with pytest.raises(ValueError, match="Either index or value subset"):
        ragged_subset_plan(sizes, 3, subset_by_index=(0, 3), subset_by_value=(0.0, 1.0), max_modes=4)
    with pytest.raises(ValueError, match="max_modes applies to subset_by_value only"):
        ragged_subset_plan(sizes, 3, max_modes=4)
    with pytest.raises(ValueError, match="max_modes applies to subset_by_value only"):
        ragged_subset_plan(sizes, 3, subset_by_index=(0, 3), max_modes=4)
    with pytest.raises(ValueError, match="needs max_modes"):
        ragged_subset_plan(sizes, 3, subset_by_value=(0.0, 1.0))
    with pytest.raises(ValueError, match="bounds are not valid"):
        ragged_subset_plan(sizes, 3, subset_by_value=(1.0, 1.0), max_modes=4)
    with pytest.raises(ValueError, match="no structures"):
        ragged_subset_plan([], 3)


def test_solver_checks_before_it_touches_the_device():
    """The constructor validates first: these raise on a machine without a GPU or a compiled library."""
    from springcraft_amd.batch import RaggedBatchSolver

    with pytest.raises(ValueError, match="smallest structure"):
        RaggedBatchSolver([43, 37], None, subset_by_index=(0, 111))
    with pytest.raises(ValueError, match="needs max_modes"):
        RaggedBatchSolver([43, 37], None, subset_by_value=(0.0, 1.0))


# ---- 2. mode_subset of a ragged batch: batch_mode_rows with m = dim * min(sizes) --------------------------------------------
@pytest.mark.parametrize("dim,ntriv", [(3, 6), (1, 1)])
def test_mode_subset_against_the_smallest_structure(dim, ntriv):
    sizes = [43, 50, 37, 64]
    m = dim * min(sizes)
    with pytest.raises(ValueError, match="Trivial modes"):
        batch_mode_rows([ntriv - 1, ntriv + 2], ntriv, None, m)
    # a mode the smallest structure does not have is an error, not silently dropped for that structure
    with pytest.raises(ValueError, match=f"mode {m} was not solved"):
        batch_mode_rows([ntriv, m], ntriv, None, m)
    rows = batch_mode_rows([m - 1, ntriv + 3, ntriv, ntriv + 3], ntriv, None, m)
    assert rows.dtype == np.int32 and rows.tolist() == [m - 1, ntriv + 3, ntriv, ntriv + 3]
    # behind an index range the rows are relative to lo, and modes outside it were not solved
    lo, hi = ragged_subset_plan(sizes, dim, subset_by_index=(ntriv, ntriv + 19))["subset"]
    rows = batch_mode_rows([ntriv + 5, ntriv, ntriv + 5], ntriv, (lo, hi), m)
    assert rows.tolist() == [5, 0, 5]
    with pytest.raises(ValueError, match="was not solved"):
        batch_mode_rows([hi + 1], ntriv, (lo, hi), m)
    # behind a window the selection is the window
    assert batch_mode_rows(None, ntriv, None, m, window=(0.0, 1.0)) is None
    with pytest.raises(ValueError, match="cannot be combined"):
        batch_mode_rows([ntriv], ntriv, None, m, window=(0.0, 1.0))


# ---- 3. solve_ragged(..., subset_by_index) -----------------------------------------------------------------------------------
SIZES = [14, 9, 14, 11, 7, 9]


def _coords():
    from oracle import enm_oracle as orc

    return [orc.synthetic_coord(n, 20 + k, 10.0) for k, n in enumerate(SIZES)]


def oracle_factory(n_atoms, batch):
    """The factory contract of solve_ragged: (batch, n_atoms, 3) -> full spectra (batch, 3 n_atoms)."""
    from oracle import enm_oracle as orc

    def run(coords):
        assert coords.shape == (batch, n_atoms, 3)
        return np.array([orc.eigen(orc.compute_hessian(c, orc.invariant_ff(8.0))[0])[0] for c in coords]), None
    return run


def _expected(lo, hi):
    from oracle import enm_oracle as orc

    return [orc.eigen(orc.compute_hessian(c, orc.invariant_ff(8.0))[0])[0][lo: hi + 1] for c in _coords()]


def test_solve_ragged_subset_single_process():
    got = solve_ragged(_coords(), None, solver_factory=oracle_factory, subset_by_index=(6, 15))
    assert len(got) == len(SIZES)
    for g, e in zip(got, _expected(6, 15)):
        assert g.shape == (10,) and np.array_equal(g, e)
    # without a subset nothing changes
    full = solve_ragged(_coords(), None, solver_factory=oracle_factory)
    assert [len(f) for f in full] == [3 * n for n in SIZES]
    assert solve_ragged([], None, solver_factory=oracle_factory, subset_by_index=(6, 15)) == []
    with pytest.raises(ValueError, match=r"smallest structure \(4: 7 atoms\)"):
        solve_ragged(_coords(), None, solver_factory=oracle_factory, subset_by_index=(6, 21))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, queue):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = {}
    coords = _coords() if rank == 0 else None
    out = solve_ragged(coords, None, solver_factory=oracle_factory, subset_by_index=(6, 15))
    seen["subset"] = out if rank == 0 else sorted(out)
    try:
        solve_ragged(coords, None, solver_factory=oracle_factory, subset_by_index=(6, 21))
        seen["beyond"] = "no error"
    except ValueError as e:
        seen["beyond"] = str(e)
    seen["empty"] = solve_ragged([] if rank == 0 else None, None, solver_factory=oracle_factory, subset_by_index=(6, 15))
    dist.barrier()      # every call left the collectives matched: one more still works
    queue.put((rank, seen))
    dist.destroy_process_group()


def test_solve_ragged_subset_two_gloo_ranks():
    import torch.multiprocessing as mp

    from springcraft_amd.batch import partition_lpt

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for g, e in zip(got[0]["subset"], _expected(6, 15)):
        assert g.shape == (10,) and np.array_equal(g, e)
    assert got[1]["subset"] == partition_lpt([float(n) ** 3 for n in SIZES], 2)[1]
    for r in (0, 1):
        assert "smallest structure (4: 7 atoms)" in got[r]["beyond"]
    assert got[0]["empty"] == [] and got[1]["empty"] == {}
