"""
CPU-only checks of the layouts behind the batch solvers' mode consumers (``batch._UniformLayout`` for
:class:`DeviceBatchSolver`, ``batch._RaggedLayout`` for :class:`RaggedBatchSolver`): buffer shapes, the offsets, shapes and
aliasing of the views handed back, the ``row_limits`` cut of per-row tensors, the displacement shape checks with their
messages, and that the table of C entries names every consumer symbol once.  Ragged sizes (3, 5, 4) against a uniform
batch of 3 structures of 4 atoms, dim 1 and 3; CPU torch tensors filled with ``arange``, so a value is its own offset.
"""
import numpy as np
import pytest
import torch

from springcraft_amd import _hip, batch
from springcraft_amd.batch import _RaggedLayout, _UniformLayout, ragged_subset_plan

SIZES = (3, 5, 4)
BATCH, N_ATOMS = 3, 4
DIMS = (1, 3)


def arange(shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float64).reshape(shape)


def aliases(view, buf):
    """``view`` is memory of ``buf``: same storage, and writing through it shows in ``buf``."""
    return view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()


def ragged(dim, **subset):
    return _RaggedLayout(SIZES, dim, ragged_subset_plan(SIZES, dim, **subset)["row_limits"])


@pytest.mark.parametrize("dim", DIMS)
def test_layouts_need_no_device_and_say_which_entries_they_take(dim):
    assert _UniformLayout(BATCH, N_ATOMS, dim).ragged is False and ragged(dim).ragged is True
    lay = ragged(dim)
    assert lay.atom_off == [0, 3, 8, 12] and lay.sq_off == [0, 9, 34, 50]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("tail", [(), (6,)])
def test_per_atom_buffers(dim, tail):
    uni = _UniformLayout(BATCH, N_ATOMS, dim)
    assert uni.atoms_shape(tail) == (BATCH, N_ATOMS) + tail
    buf = arange(uni.atoms_shape(tail))
    assert uni.atoms_out(buf) is buf

    lay = ragged(dim)
    assert lay.atoms_shape(tail) == (sum(SIZES),) + tail
    buf = arange(lay.atoms_shape(tail))
    per = int(np.prod(tail, dtype=np.int64))
    views = lay.atoms_out(buf)
    assert isinstance(views, list) and len(views) == len(SIZES)
    for b, (n, view) in enumerate(zip(SIZES, views)):
        assert tuple(view.shape) == (n,) + tail
        assert view.reshape(-1)[0].item() == sum(SIZES[:b]) * per       # starts at atom sum(sizes[:b])
        assert aliases(view, buf) and view.storage_offset() == sum(SIZES[:b]) * per and view.is_contiguous()
    views[1].zero_()
    assert not buf[3:8].any() and buf[:3].any() and buf[8:].all()


@pytest.mark.parametrize("dim", DIMS)
def test_per_pair_buffers(dim):
    uni = _UniformLayout(BATCH, N_ATOMS, dim)
    assert uni.pairs_shape() == (BATCH, N_ATOMS, N_ATOMS)
    buf = arange(uni.pairs_shape())
    assert uni.pairs_out(buf) is buf
    scale = arange(uni.atoms_shape())
    assert [(c is buf, s is scale) for c, s in uni.pair_blocks(buf, scale)] == [(True, True)]
    assert [(c is buf, s) for c, s in uni.pair_blocks(buf, None)] == [(True, None)]

    lay = ragged(dim)
    assert lay.pairs_shape() == (sum(n * n for n in SIZES),)
    buf = arange(lay.pairs_shape())
    views = lay.pairs_out(buf)
    assert isinstance(views, list) and len(views) == len(SIZES)
    for b, (n, view) in enumerate(zip(SIZES, views)):
        start = sum(k * k for k in SIZES[:b])
        assert tuple(view.shape) == (n, n) and view[0, 0].item() == start and view[1, 0].item() == start + n
        assert aliases(view, buf) and view.storage_offset() == start and view.is_contiguous()
    # the post-processing blocks: every structure's view with its own cut of a packed atom_scale, or None
    scale = arange(lay.atoms_shape())
    blocks = list(lay.pair_blocks(views, scale))
    assert len(blocks) == len(SIZES)
    for b, (c, s) in enumerate(blocks):
        assert c is views[b] and tuple(s.shape) == (SIZES[b],) and s[0].item() == sum(SIZES[:b]) and aliases(s, scale)
    assert [s for _, s in lay.pair_blocks(views, None)] == [None] * len(SIZES)
    views[2].zero_()
    assert not buf[34:].any() and buf[1:34].all()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("subset", ["full", "index", "window"])
def test_per_row_tensors_are_cut_by_row_limits(dim, subset):
    own_min = dim * min(SIZES)
    if subset == "full":
        kw, nvec, limits = {}, dim * max(SIZES), [dim * n for n in SIZES]
    elif subset == "index":
        kw, nvec, limits = {"subset_by_index": (1, own_min - 1)}, own_min - 1, [own_min - 1] * len(SIZES)
    else:
        kw, nvec, limits = {"subset_by_value": (0.5, np.inf), "max_modes": 2}, 2, [2] * len(SIZES)
    lay = ragged(dim, **kw)
    assert lay.row_limits == limits
    q = 2
    rows, multi = arange((len(SIZES), nvec)), arange((len(SIZES), q, nvec))
    for b, (r, one, many, first) in enumerate(zip(limits, lay.rows_out(rows), lay.rows_out(multi),
                                                  lay.rows_out(multi[:, :1].contiguous(), single=True))):
        assert tuple(one.shape) == (r,) and one[0].item() == b * nvec and aliases(one, rows)
        assert tuple(many.shape) == (q, r) and many[0, 0].item() == b * q * nvec and many[1, 0].item() == (b * q + 1) * nvec
        assert aliases(many, multi)
        assert tuple(first.shape) == (r,)
    empty = lay.rows_out(torch.empty((len(SIZES), 0, nvec), dtype=torch.float64))
    assert [tuple(e.shape) for e in empty] == [(0, r) for r in limits]

    uni = _UniformLayout(BATCH, N_ATOMS, dim)
    rows, multi = arange((BATCH, nvec)), arange((BATCH, q, nvec))
    assert uni.rows_out(rows) is rows and uni.rows_out(multi) is multi
    one = uni.rows_out(multi[:, :1], single=True)
    assert tuple(one.shape) == (BATCH, nvec) and torch.equal(one, multi[:, 0])


@pytest.mark.parametrize("dim", DIMS)
def test_displacement_shapes(dim):
    xyz = (3,) if dim == 3 else ()
    uni = _UniformLayout(BATCH, N_ATOMS, dim)
    lead, tail, names = uni.displacement()
    assert lead == (BATCH,) and tail == (N_ATOMS,) + xyz
    assert names == ("(batch, N, 3) or (batch, q, N, 3)" if dim == 3 else "(batch, N) or (batch, q, N)") + \
        f" with batch = {BATCH}, N = {N_ATOMS}"
    assert uni.displacement_q(lead + tail) == (1, True)
    for q in (0, 1, 2):
        assert uni.displacement_q(torch.empty(lead + (q,) + tail).shape) == (q, False)
    for bad in [(BATCH, N_ATOMS + 1) + xyz, (BATCH, 2, N_ATOMS + 1) + xyz, (BATCH + 1, N_ATOMS) + xyz, (N_ATOMS,) + xyz,
                (BATCH, 2, 2, N_ATOMS) + xyz]:
        with pytest.raises(ValueError) as e:
            uni.displacement_q(bad)
        assert str(e.value) == f"Expected a displacement of shape {names}, got {bad}"

    lay = ragged(dim)
    total = sum(SIZES)
    lead, tail, names = lay.displacement()
    assert lead == () and tail == (total,) + xyz
    assert names == ("(S, 3) or (q, S, 3)" if dim == 3 else "(S,) or (q, S)") + f" with S = sum(sizes) = {total}"
    assert lay.displacement_q(tail) == (1, True)
    for q in (0, 1, 2):
        assert lay.displacement_q((q,) + tail) == (q, False)
    for bad in [(total + 1,) + xyz, (2, total + 1) + xyz, (2, 2, total) + xyz, (BATCH, N_ATOMS) + xyz]:
        with pytest.raises(ValueError) as e:
            lay.displacement_q(bad)
        assert str(e.value) == f"Expected a displacement of shape {names}, got {bad}"
    # coord and atom_scale are per-atom buffers with tails (3,) and ()
    assert uni.atoms_shape((3,)) == (BATCH, N_ATOMS, 3) and lay.atoms_shape((3,)) == (total, 3) and lay.atoms_shape() == (total,)


def test_the_entry_table_names_every_consumer_symbol_once():
    names = [n for row in batch._CONSUMER_ENTRIES.values() for n in (row[0], row[2])]
    assert len(names) == len(set(names)) == 10
    assert set(names) == {s for s in _hip.EXPORTED_SYMBOLS
                          if s.startswith(("sc_dev_modes_", "sc_batch_plan_modes_")) and not s.endswith("workspace_bytes")}
    source = open(batch.__file__).read()
    for n in names:
        assert source.count(n) == 1, n
    for uniform, uniform_prefix, plan, plan_prefix in batch._CONSUMER_ENTRIES.values():
        assert uniform.startswith("sc_dev_modes_") and uniform_prefix[0] == "ctx"
        assert plan == uniform.replace("sc_dev_modes_", "sc_batch_plan_modes_") and plan_prefix[0] == "plan"
    # neither solver class has a consumer body of its own
    for cls in (batch.DeviceBatchSolver, batch.RaggedBatchSolver):
        for name in ("frequencies", "mean_square_fluctuation", "bfactor", "_aniso_packed", "anisotropic_fluctuation", "overlap",
                     "collectivity", "distance_fluctuation", "dcc", "_selection"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(batch._BatchSolver, name)
