"""
Times of the pair-list operator (springcraft_amd.PairOperator, csrc/pair_operator.hip) for profiles/pair_operator.txt.
Needs an MI355X; reads nothing but the package and bench.py's structure generator.

    python tools/pair_operator_timing.py [--out profiles/pair_operator.txt] [--large 50000] [--repeat 5] [--skip-small]

N = 8000 C-alpha (the C5 structure of bench.py, seed 0, InvariantForceField 13 A), 106 standard-normal rows:
  * ``apply``, ``energy``, ``apply_energy`` and the strain of every spring from stream events, median of --repeat runs after
    one warm-up run, with the pairs x rows per second they amount to
  * torch's dense ``H @ X^T`` on the (24000, 24000) Hessian of ``compute_hessian`` uploaded to the device, same events,
    and the largest difference of the two products
and one size the dense Hessian cannot exist at (--large atoms, blocks of 10 consecutive atoms, modes 0..105):
``RTB.residuals()`` against ``RTB.solve()``, stream events, with the residuals of modes 6..15 and w of the same modes.
No gate: the figures are for the README.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import springcraft_amd as sc  # noqa: E402

ROWS = 106
SUBSET = (0, 105)


def timed(torch, fn, repeat):
    """Stream-event times in ms of ``repeat`` runs of ``fn`` after one warm-up run, and the last result."""
    times, out = [], None
    for it in range(repeat + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if it:
            times.append(a.elapsed_time(b))
    return times, out


def line(name, times, work=None):
    rate = f"  {work / np.median(times) / 1e6:8.2f} G pair-rows/s" if work else ""
    return f"  {name:34s} median {np.median(times):9.3f} ms  (min {min(times):.3f}, max {max(times):.3f}, {len(times)} runs){rate}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_operator.txt"))
    ap.add_argument("--large", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-small", action="store_true", help="only the --large case")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pair_operator_timing.py measures on the GPU: no device found")
    lines = [f"tools/pair_operator_timing.py --large {args.large} --repeat {args.repeat}", sc._hip.context().info(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def flush():   # after every section: a later one that fails leaves the earlier figures
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    ff = sc.InvariantForceField(13.0)
    if not args.skip_small:
        coord = bench.synthetic_coords(8000, [0])[0]
        op = sc.PairOperator(coord, ff)
        x = torch.from_numpy(np.random.RandomState(0).standard_normal((ROWS, 3 * len(coord)))).cuda()
        work = op.n_pairs * ROWS
        per_atom = np.diff(sc.pair_operator.pair_row_start(op.pairs, op.n_atoms))
        lines.append(f"N = {op.n_atoms}, {op.n_pairs} directed pairs ({per_atom.mean():.1f} per atom, {per_atom.min()} .. "
                     f"{per_atom.max()}), {ROWS} rows")
        t_apply, y = timed(torch, lambda: op.apply(x), args.repeat)
        lines.append(line("apply (Y)", t_apply, work))
        lines.append(line("energy (E)", timed(torch, lambda: op.energy(x), args.repeat)[0], work))
        lines.append(line("apply_energy (Y and E)", timed(torch, lambda: op.apply_energy(x), args.repeat)[0], work))
        lines.append(line("strain, every spring once", timed(torch, lambda: op.strain(x), args.repeat)[0], work // 2))
        flush()
        h = torch.from_numpy(sc.compute_hessian(coord, ff)[0]).cuda()
        t_dense, dense = timed(torch, lambda: x @ h.T, args.repeat)
        lines.append(line(f"torch dense H @ X^T, order {h.shape[0]}", t_dense))
        lines.append(f"  apply / dense: {np.median(t_apply) / np.median(t_dense):.3f};  max |Y - dense| = "
                     f"{float((y - dense).abs().max()):.3e} at max |Y| = {float(y.abs().max()):.3e}")
        lines.append("")
        del h, dense, y, x, op
        torch.cuda.empty_cache()
        flush()

    if args.large:
        big = bench.synthetic_coords(args.large, [0])[0]
        rtb = sc.RTB(big, ff, sc.blocks_of_consecutive(args.large, 10))
        lines.append(f"a size the dense Hessian cannot exist at: N = {args.large} (dense Hessian {9 * args.large**2 * 8 / 1e9:.0f} GB), "
                     f"blocks of 10 consecutive atoms, nr = {rtb.nr}, {rtb.n_pairs} directed pairs, modes {SUBSET[0]}..{SUBSET[1]}")
        repeat = max(1, min(args.repeat, 2))
        t_solve, _ = timed(torch, lambda: rtb.solve(subset_by_index=SUBSET), repeat)
        rtb.finish()
        lines.append(line("RTB.solve()", t_solve))
        _ = rtb.operator   # (built once: row starts and the symmetry check on the host)
        t_res, res = timed(torch, rtb.residuals, repeat)
        lines.append(line("RTB.residuals()", t_res, rtb.n_pairs * rtb.nvec))
        lines.append(line("RTB.deformation_energy()", timed(torch, rtb.deformation_energy, repeat)[0], rtb.n_pairs * (rtb.nvec - 6)))
        lines.append(f"  residuals / solve: {np.median(t_res) / np.median(t_solve):.4f}")
        w = rtb.w[0].cpu().numpy()
        lines.append("  w[6:16]:         " + " ".join(f"{v:.4e}" for v in w[6:16]))
        lines.append("  residuals[6:16]: " + " ".join(f"{v:.4e}" for v in res.cpu().numpy()[6:16]))
        lines.append("  residuals[0:6]:  " + " ".join(f"{v:.4e}" for v in res.cpu().numpy()[:6]))
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
