"""
Times of the conjugate-gradient kernels (csrc/pair_cg.hip) and of the solves built on them (PairOperator.solve,
RTB.exact_response) for profiles/pair_cg.txt.  Needs an MI355X; reads nothing but the package and bench.py's structure
generator.

    python tools/solve_timing.py [--out profiles/pair_cg.txt] [--large 50000] [--repeat 5] [--tol 1e-8] [--skip-small]
                                 [--skip-dense]

The structures of tools/iterative_timing.py: N = 8000 C-alpha (bench.py's generator, seed 0, InvariantForceField 13 A) and
--large atoms of the same generator.
  * one CG iteration (``sc_dev_pairs_cg_step_f64``, 20 iterations per timed call) against one panel step ``Z <- H X`` on the
    same panel, stream events, median of --repeat runs after a warm-up run, q = 64 and 128.  By bytes an iteration is one
    panel step plus about eight streamed panel passes (update: four reads, two writes; direction: two reads, one write, less
    the Q write the panel step has too): the model time is the panel step plus 8 passes of 8 m q bytes at the measured
    copy rate of a (m, q) panel.
  * ``PairOperator.solve`` of 128 standard-normal forces to --tol: iterations and time, undeflated and deflated with the 106
    modes of ``RTB.refine``; at N = 8000 the largest difference to ``nma.linear_response`` of the dense ``ANM``
  * ``RTB.exact_response`` against the truncated ``RTB.linear_response`` on the same 106 modes
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
from tools.iterative_timing import SUBSET, cubic_cells  # noqa: E402
from tools.pair_operator_timing import timed  # noqa: E402

CG_PER_CALL = 20


def iteration_against_panel_step(torch, op, q, repeat, lines):
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((op.m, q))).cuda()
    z = torch.empty_like(x)
    t_panel, _ = timed(torch, lambda: op.panel_step(x, z, 1.0, 0.0, 0.0), repeat)
    t_copy, _ = timed(torch, lambda: z.copy_(x), repeat)

    def iterations():
        init, step = op._cg_callables(q)
        init(x.clone(), 1e-30)
        return step

    step = iterations()
    t_cg, _ = timed(torch, lambda: step(CG_PER_CALL), repeat)
    panel, copy, cg = np.median(t_panel), np.median(t_copy), np.median(t_cg) / CG_PER_CALL
    model = panel + 8 * copy / 2   # (a copy moves two panels)
    lines.append(f"N = {op.n_atoms}, {op.n_pairs} directed pairs, q = {q}: panel step {panel:.3f} ms, copy of one panel "
                 f"{copy:.3f} ms ({2 * 8 * op.m * q / copy / 1e6:.0f} GB/s), one CG iteration {cg:.3f} ms")
    lines.append(f"  CG iteration / panel step = {cg / panel:.2f}; byte model (panel step + 8 streamed passes) {model:.3f} ms: "
                 f"measured / model = {cg / model:.2f}")


def solves(torch, rtb, tol, lines, dense=None):
    op, n = rtb.operator, rtb.n_atoms
    force = np.random.RandomState(1).standard_normal((128, n, 3))

    def run(label, call):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        x, info = call()
        b.record()
        torch.cuda.synchronize()
        lines.append(f"  {label}: converged {info['converged']}, iterations {info['iterations'].min()}..{info['iterations'].max()}, "
                     f"{a.elapsed_time(b):.1f} ms, max residual {info['residuals'].max():.2e}")
        return x

    rtb.solve(subset_by_index=SUBSET)
    rtb.finish()
    x_plain = run(f"exact_response, 128 forces, tol {tol:g}, undeflated", lambda: rtb.exact_response(force, tol=tol))
    info = rtb.refine(tol=tol)
    lines.append(f"  RTB.refine(tol={tol:g}) of modes {SUBSET[0]}..{SUBSET[1]}: converged {info['converged']}, lambda_6 = "
                 f"{float(rtb.w[0, 6]):.4g}, lambda_105 = {float(rtb.w[0, -1]):.4g}, b = {info['b']:.4g}")
    x = run(f"exact_response, deflated with the {rtb.nvec} refined modes", lambda: rtb.exact_response(force, tol=tol))
    lines.append(f"  deflated against undeflated: max |dx| = {float((x - x_plain).abs().max()):.3e} at max |x| = {float(x.abs().max()):.3e}")
    trunc = rtb.linear_response(torch.from_numpy(force).cuda()[None])[0]
    num = torch.linalg.vector_norm((trunc - x).reshape(128, -1), dim=1)
    rel = (num / torch.linalg.vector_norm(x.reshape(128, -1), dim=1)).cpu().numpy()
    lines.append(f"  truncated RTB.linear_response on the same {rtb.nvec - 6} modes: |dx_truncated - dx_exact| / |dx_exact| = "
                 f"{rel.min():.3f} .. {rel.max():.3f} (median {np.median(rel):.3f})")
    if dense is not None:
        ref = np.stack([sc.nma.linear_response(dense, f) for f in force[:8]])
        lines.append(f"  against nma.linear_response of the dense ANM (8 forces): max |dx| = "
                     f"{np.abs(x[:8].cpu().numpy() - ref).max():.3e} at max |x| = {np.abs(ref).max():.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_cg.txt"))
    ap.add_argument("--large", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--skip-small", action="store_true", help="only the --large cases")
    ap.add_argument("--skip-dense", action="store_true", help="no dense ANM to compare the response with")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("solve_timing.py measures on the GPU: no device found")
    lines = [f"tools/solve_timing.py --large {args.large} --repeat {args.repeat} --tol {args.tol:g}", sc._hip.context().info(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def flush():   # after every section: a later one that fails leaves the earlier figures
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    ff = sc.InvariantForceField(13.0)
    cases = []
    if not args.skip_small:
        small = bench.synthetic_coords(8000, [0])[0]
        cases.append((small, cubic_cells(small, 10.0), not args.skip_dense))
    if args.large:
        cases.append((bench.synthetic_coords(args.large, [0])[0], sc.blocks_of_consecutive(args.large, 10), False))
    for coord, labels, dense in cases:
        rtb = sc.RTB(coord, ff, labels)
        for q in (64, 128):
            iteration_against_panel_step(torch, rtb.operator, q, args.repeat, lines)
        flush()
        solves(torch, rtb, args.tol, lines, sc.ANM(coord, ff) if dense else None)
        lines.append("")
        flush()
        del rtb
        torch.cuda.empty_cache()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
