"""
Phase times and accuracy of the rotation-translation-block modes (springcraft_amd.RTB) against the dense partial-spectrum
solve, for profiles/rtb.txt.  Needs an MI355X; reads nothing but the package and bench.py's structure generator.

    python tools/rtb_timing.py [--out profiles/rtb.txt] [--large 50000] [--repeat 5] [--skip-dense] [--skip-small]

N = 8000 C-alpha (the C5 structure of bench.py, seed 0, InvariantForceField 13 A), blocks of 5 and of 10 consecutive
residues and, since that structure is a random cloud without a chain, cubic cells of 5 and of 10 atoms on average; modes
0..105 (6 trivial + 100):
  * setup on the host clock (it ends in synchronising calls): projector, pair list, gamma, upload + key sort
  * projection, eigensolve, expansion from stream events, median of --repeat runs after one warm-up run
  * ``ANM.eigen(subset_by_index=(0, 105))`` of the same structure on the host clock, same number of runs
  * overlap of each of the first 20 non-trivial RTB modes with the span of the first 40 non-trivial full modes, and
    lambda_rtb / lambda_full
and one size the dense path cannot hold (--large atoms, blocks of 10, modes 0..105) with the peak device memory.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import springcraft_amd as sc  # noqa: E402

SUBSET = (0, 105)


def median(xs):
    return float(np.median(np.asarray(xs)))


def cell_blocks(coord, mean_atoms):
    """Labels of cubic cells sized for ``mean_atoms`` atoms on average: spatially compact blocks, not contiguous in atom order."""
    n = len(coord)
    extent = coord.max(axis=0) - coord.min(axis=0)
    edge = (np.prod(extent) * mean_atoms / n) ** (1.0 / 3.0)
    cell = np.floor((coord - coord.min(axis=0)) / edge).astype(np.int64)
    return (cell[:, 0] * 100003 + cell[:, 1]) * 100003 + cell[:, 2]


def timed_rtb(torch, coord, block_size, repeat, lines, cells=False):
    n = len(coord)
    ff = sc.InvariantForceField(13.0)
    labels = cell_blocks(coord, block_size) if cells else sc.blocks_of_consecutive(n, block_size)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    P = sc.rtb_projector(coord, labels)
    t_proj_host = time.perf_counter() - t0
    del P
    t0 = time.perf_counter()
    rtb = sc.RTB(coord, ff, labels)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    what = f"cubic cells of {block_size} atoms on average" if cells else f"blocks of {block_size} consecutive atoms"
    lines.append(f"N = {n}, {what}: {rtb.n_blocks} blocks, nr = {rtb.nr}, {rtb.n_pairs} directed pairs, "
                 f"{rtb.n_segments} block-pair segments")
    lines.append(f"  setup, host clock: {t_setup * 1e3:9.1f} ms  (projector on the host {t_proj_host * 1e3:.1f} ms of it; the rest: "
                 "contact scan + pair list, gamma on the host, uploads, key sort)")
    # the separate phases of the setup, once more, on the host clock
    from springcraft_amd.forcefield import device_plan
    from springcraft_amd.interaction import _pair_list

    t0 = time.perf_counter()
    pairs, sq = _pair_list(rtb.ctx, rtb.coord, device_plan(ff)[0], None, True)
    t_pairs = time.perf_counter() - t0
    t0 = time.perf_counter()
    ff.force_constant(pairs[:, 0], pairs[:, 1], sq)
    t_gamma = time.perf_counter() - t0
    lines.append(f"    pair list (device scan, copied back): {t_pairs * 1e3:9.1f} ms   gamma on the host: {t_gamma * 1e3:9.1f} ms")
    del pairs, sq

    phases = {"projection": [], "eigensolve": [], "expansion": [], "solve": []}
    wall = []
    for it in range(repeat + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        rtb.subset, rtb.nvec, rtb._first_row = SUBSET, SUBSET[1] - SUBSET[0] + 1, SUBSET[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        rtb.assemble()
        ev[1].record()
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        rtb.ctx.check(rtb._L.sc_dev_eigh_range_f64(rtb.ctx.handle, p(rtb.matrix), rtb.nr, 1, SUBSET[0], SUBSET[1], p(rtb.w),
                                                   p(rtb._u)))
        ev[2].record()
        rtb.ctx.check(rtb._L.sc_dev_rtb_expand_f64(rtb.ctx.handle, p(rtb._u), rtb.nvec, rtb.nr, p(rtb._P), p(rtb._boa),
                                                   p(rtb._offset), rtb.n_atoms, p(rtb.v)))
        ev[3].record()
        rtb.finish()
        dt = time.perf_counter() - t0
        if it == 0:
            continue     # warm-up: workspace allocation, code objects
        wall.append(dt * 1e3)
        phases["projection"].append(ev[0].elapsed_time(ev[1]))
        phases["eigensolve"].append(ev[1].elapsed_time(ev[2]))
        phases["expansion"].append(ev[2].elapsed_time(ev[3]))
        phases["solve"].append(ev[0].elapsed_time(ev[3]))
    for name in ("projection", "eigensolve", "expansion", "solve"):
        xs = phases[name]
        lines.append(f"  {name:11s} stream events: median {median(xs):9.3f} ms  (min {min(xs):.3f}, max {max(xs):.3f}, {len(xs)} runs)")
    lines.append(f"  solve() + finish(), host clock: median {median(wall):9.3f} ms")
    free, total = torch.cuda.mem_get_info()
    lines.append(f"  device memory: peak held by torch tensors {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB; in use on the device "
                 f"after the solves, all allocators (the eigensolver's cached workspace included): {(total - free) / 2**30:.2f} GiB")
    w, v = rtb.w[0].cpu().numpy(), rtb.v[0].cpu().numpy()
    return w, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtb.txt"))
    ap.add_argument("--large", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--skip-small", action="store_true", help="only the --large case")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rtb_timing.py measures on the GPU: no device found")
    lines = [f"tools/rtb_timing.py --large {args.large} --repeat {args.repeat}", sc._hip.context().info(), ""]
    coord = bench.synthetic_coords(8000, [0])[0]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def flush():   # after every section: a later one that fails leaves the earlier figures
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    results = {}
    # (the synthetic structure is a uniform random cloud: consecutive atoms are not neighbours in space, as they are along
    # a chain, so consecutive blocks are scattered and stiff there; the cell blocks show compact blocks of the same sizes)
    for key in () if args.skip_small else ((5, False), (10, False), (5, True), (10, True)):
        results[key] = timed_rtb(torch, coord, key[0], args.repeat, lines, cells=key[1])
        lines.append("")
        flush()

    if not args.skip_dense and not args.skip_small:
        ff = sc.InvariantForceField(13.0)
        dense = []
        for it in range(args.repeat + 1):
            t0 = time.perf_counter()
            w_full, v_full = sc.ANM(coord, ff).eigen(subset_by_index=SUBSET)
            if it:
                dense.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"dense path, ANM.eigen(subset_by_index={SUBSET}), N = 8000, order 24000, host clock (result on the host): "
                     f"median {median(dense):.1f} ms  (min {min(dense):.1f}, max {max(dense):.1f}, {len(dense)} runs)")
        lines.append("")
        span = v_full[6:46]
        for (bs, cells), (w, v) in results.items():
            ov = np.sqrt(((v[6:26] @ span.T) ** 2).sum(axis=1))
            ratio = w[6:26] / w_full[6:26]
            lines.append(f"{'cells' if cells else 'consecutive blocks'} of {bs}: RTB modes 6..25 against the dense modes")
            lines.append("  overlap with span(dense modes 6..45): " + " ".join(f"{x:.3f}" for x in ov))
            lines.append("  lambda_rtb / lambda_full:             " + " ".join(f"{x:.3f}" for x in ratio))
        lines.append("")
        del v_full
        flush()

    if args.large:
        big = bench.synthetic_coords(args.large, [0])[0]
        lines.append(f"a size the dense path cannot hold: N = {args.large} (dense Hessian {9 * args.large**2 * 8 / 1e9:.0f} GB)")
        timed_rtb(torch, big, 10, max(1, min(args.repeat, 2)), lines)
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
