"""
Timing of the generalized correlation (csrc/mode_lmi.hip) against perturbation-response scanning with stream events.

    python tools/lmi_timing.py [--quick] >> profiles/lmi.txt

generalized_correlation() and generalized_correlation(information=True) against prs(norm=False) of the same solver and
selection: the three read the same rows and issue the same MFMAs (18 flops per pair and row); the generalized correlation
adds the diagonal blocks (the anisotropic-tensor kernels, one more pass over the selected rows), the whitening and an
epilogue of about 180 flops and two or three transcendental calls per pair.

1. 64 structures of N = 2000, all non-trivial modes and the 20 lowest;
2. one model of N = 2000, all non-trivial modes.

The tensors are not solved: w is positive and v random (tools/prs_timing.py), which costs the kernels what eigenvectors cost
them and leaves every diagonal block positive definite.  Every figure is the median of `--repeat` runs after one warm-up,
events on the solver's stream around the whole call (weights, tensors, whitening and pair kernel).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.prs_timing import fake_modes, median_ms, tile_flops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 300 and a batch of 4: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip
    from springcraft_amd.batch import DeviceBatchSolver

    print(f"# tools/lmi_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    ff = sc.InvariantForceField(13.0)
    print("#    shape, selection                      prs(norm=False)   TFLOP/s   r      r / prs   I      I / prs   (ms)")
    batch, n = (4, 300) if args.quick else (64, 2000)
    for nb in (batch, 1):
        s = DeviceBatchSolver(n, nb, ff)
        s.matrix = None                                       # (nothing is solved here)
        torch.cuda.empty_cache()
        fake_modes(torch, s, 1)
        cases = [("all non-trivial modes", None, 3 * n)]
        if nb > 1:
            cases.append(("20 modes (6..25)", np.arange(6, 26), 20))
        for name, subset, rows in cases:
            prs = median_ms(torch, lambda: s.prs(subset, norm=False), args.repeat)
            r = median_ms(torch, lambda: s.generalized_correlation(subset), args.repeat)
            info = median_ms(torch, lambda: s.generalized_correlation(subset, information=True), args.repeat)
            out = s.generalized_correlation(subset)
            assert bool(torch.isfinite(out).all())
            print(f"  {nb:3d} x N = {n}, {name:22s} {prs:10.3f}   {tile_flops(n, rows, nb) / prs * 1e-9:8.2f}   {r:10.3f}   "
                  f"{r / prs:6.3f}   {info:10.3f}   {info / prs:6.3f}")
        del s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
