"""
Times of the column-panel step (csrc/pair_panel.hip) and of the Chebyshev-filtered subspace iteration built on it
(springcraft_amd/iterative.py, PairOperator.lowest_modes, RTB.refine) for profiles/iterative_modes.txt.  Needs an MI355X;
reads nothing but the package and bench.py's structure generator.

    python tools/iterative_timing.py [--out profiles/iterative_modes.txt] [--large 50000] [--repeat 5] [--tol 1e-8]
                                     [--skip-small] [--skip-dense]

The structures of tools/pair_operator_timing.py: N = 8000 C-alpha (the C5 structure of bench.py, seed 0,
InvariantForceField 13 A) and --large atoms of the same generator.
  * one panel step ``Z <- H X`` on q standard-normal columns against ``PairOperator.apply`` on the same vectors as rows
    (the kernel of csrc/pair_operator.hip, unchanged), stream events, median of --repeat runs after one warm-up run, with
    the largest difference of the two results: N = 8000 with q = 64 and 128, --large with q = 128
  * ``RTB.refine`` of modes 0..105 at N = 8000, blocks = cubic cells of 10 A: passes, panel steps, time (stream events
    around the whole call, its host synchronisations included), and the largest ``|w - w_dense| / b`` against
    ``ANM.eigen(subset_by_index=(0, 105))`` (--skip-dense leaves the dense solve out)
  * the same refine at --large atoms, blocks of 10 consecutive atoms: passes, time, final residuals, and the peak of
    torch's device allocations during the call (the panels and their products; the eigensolver's own workspace for the
    (nb, nb) matrices is printed next to it)
No gate: the figures are for the README and DESIGN.md.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import springcraft_amd as sc  # noqa: E402
from tools.pair_operator_timing import line, timed  # noqa: E402

SUBSET = (0, 105)


def cubic_cells(coord, edge):
    """Block labels: the cubic cell of edge ``edge`` an atom lies in."""
    cell = np.floor((coord - coord.min(axis=0)) / edge).astype(np.int64)
    span = cell.max(axis=0) + 1
    return (cell[:, 0] * span[1] + cell[:, 1]) * span[2] + cell[:, 2]


def panel_against_apply(torch, op, q, repeat, lines):
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((op.m, q))).cuda()
    rows = x.T.contiguous()
    z = torch.empty_like(x)
    work = op.n_pairs * q
    t_panel, _ = timed(torch, lambda: op.panel_step(x, z, 1.0, 0.0, 0.0), repeat)
    t_apply, y = timed(torch, lambda: op.apply(rows), repeat)
    t_rec, _ = timed(torch, lambda: op.panel_step(x, z, 0.7, -1.3, 0.4), repeat)
    op.panel_step(x, z, 1.0, 0.0, 0.0)
    lines.append(f"N = {op.n_atoms}, {op.n_pairs} directed pairs, q = {q}")
    lines.append(line("panel step, Z <- H X", t_panel, work))
    lines.append(line("panel step, full recurrence", t_rec, work))
    lines.append(line("apply on the same vectors as rows", t_apply, work))
    lines.append(f"  panel / apply: {np.median(t_panel) / np.median(t_apply):.3f};  max |Z - Y^T| = "
                 f"{float((z - y.T).abs().max()):.3e} at max |Y| = {float(y.abs().max()):.3e}")
    lines.append("")


def refine(torch, rtb, tol, lines):
    rtb.solve(subset_by_index=SUBSET)
    rtb.finish()
    _ = rtb.operator
    before = rtb.residuals().cpu().numpy()
    w_block = rtb.w[0].cpu().numpy()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    info = rtb.refine(tol=tol)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    after = rtb.residuals().cpu().numpy()
    w = rtb.w[0].cpu().numpy()
    nb = rtb.nvec + sc.iterative.default_guard(rtb.nvec)
    lines.append(f"  block modes: residuals[6:] {before[6:].min():.3e} .. {before[6:].max():.3e}, b = {info['b']:.6g}")
    lines.append(f"  RTB.refine(tol={tol:g}): converged {info['converged']}, {info['iterations']} passes, {info['panel_steps']} "
                 f"panel steps of {nb} columns, {a.elapsed_time(b):.1f} ms")
    lines.append(f"  refined: residuals {after.min():.3e} .. {after.max():.3e} (tol b = {tol * info['b']:.3e}); "
                 f"w_block / w over modes 6.. : {(w_block[6:] / w[6:]).min():.3f} .. {(w_block[6:] / w[6:]).max():.3f}")
    lines.append(f"  peak of torch's device allocations during refine: {peak / 2**20:.1f} MiB (one panel: "
                 f"{8 * rtb.m * nb / 2**20:.1f} MiB); eigensolver workspace for ({nb}, {nb}): "
                 f"{sc._hip.lib().sc_eigh_workspace_bytes(nb, 1, 1) / 2**20:.1f} MiB")
    lines.append("  w[6:16]:         " + " ".join(f"{v:.4e}" for v in w[6:16]))
    lines.append("  residuals[6:16]: " + " ".join(f"{v:.4e}" for v in after[6:16]))
    return w, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iterative_modes.txt"))
    ap.add_argument("--large", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--skip-small", action="store_true", help="only the --large cases")
    ap.add_argument("--skip-dense", action="store_true", help="no dense solve to compare the refined eigenvalues with")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("iterative_timing.py measures on the GPU: no device found")
    lines = [f"tools/iterative_timing.py --large {args.large} --repeat {args.repeat} --tol {args.tol:g}",
             sc._hip.context().info(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def flush():   # after every section: a later one that fails leaves the earlier figures
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    ff = sc.InvariantForceField(13.0)
    small = None if args.skip_small else bench.synthetic_coords(8000, [0])[0]
    big = bench.synthetic_coords(args.large, [0])[0] if args.large else None
    if small is not None:
        op = sc.PairOperator(small, ff)
        for q in (64, 128):
            panel_against_apply(torch, op, q, args.repeat, lines)
        del op
        flush()
    if big is not None:
        op = sc.PairOperator(big, ff)
        panel_against_apply(torch, op, 128, args.repeat, lines)
        del op
        flush()

    if small is not None:
        labels = cubic_cells(small, 10.0)
        rtb = sc.RTB(small, ff, labels)
        lines.append(f"RTB.refine, N = {len(small)}, cubic cells of 10 A: {rtb.n_blocks} blocks, nr = {rtb.nr}, modes "
                     f"{SUBSET[0]}..{SUBSET[1]}")
        w, info = refine(torch, rtb, args.tol, lines)
        flush()
        del rtb
        torch.cuda.empty_cache()
        if not args.skip_dense:
            t_dense, dense = timed(torch, lambda: sc.ANM(small, ff).eigen(subset_by_index=SUBSET), 1)
            lines.append(f"  ANM.eigen(subset_by_index={SUBSET}), host call with assembly and copies: {t_dense[0]:.1f} ms;  "
                         f"max |w - w_dense| / b = {np.abs(w - dense[0]).max() / info['b']:.3e}")
        lines.append("")
        flush()

    if big is not None:
        rtb = sc.RTB(big, ff, sc.blocks_of_consecutive(args.large, 10))
        lines.append(f"RTB.refine, N = {args.large} (dense Hessian {9 * args.large**2 * 8 / 1e9:.0f} GB), blocks of 10 consecutive "
                     f"atoms, nr = {rtb.nr}, {rtb.n_pairs} directed pairs, modes {SUBSET[0]}..{SUBSET[1]}")
        refine(torch, rtb, args.tol, lines)
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
