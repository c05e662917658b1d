"""
Timing of batch perturbation-response scanning (csrc/mode_prs.hip) with stream events.

    python tools/prs_timing.py [--quick] > profiles/batch_prs.txt

1. one model, N = 1000 and N = 2000, all non-trivial modes: the new kernel (a DeviceBatchSolver of one structure, events
   on its stream) against sc_modes_prs, which forms V / w and the (3N, 3N) covariance in scratch and reduces it (a host
   entry on the context's own stream that ends with the copy of the (N, N) result: wall clock, the copy included; the new
   kernel's host entry sc_modes_prs_subset is timed the same way beside it);
2. 64 structures of N = 2000, all non-trivial modes and the 20 lowest, against dcc(norm=False) of the same selection (the
   grouped GEMM of batch_consumers.hip: a third of the multiply-adds, and its operands are packed to scratch first).

The batch tensors are not solved: w is positive and v random, which costs the kernels what eigenvectors cost them.  Every
figure is the median of `--repeat` runs after one warm-up; flops are 18 per (pair, row) over the N (N + 1) / 2 pairs of the
tiles' lower triangle, counted as computed (whole 64 x 64 tiles).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times))


def tile_flops(n_atoms, rows, batch):
    t = -(-n_atoms // 64)
    return 18.0 * (t * (t + 1) // 2) * 4096 * rows * batch


def fake_modes(torch, s, seed):
    """Positive eigenvalues above six ~0 ones and random rows of unit length scale: nothing is solved."""
    g = torch.Generator(device=s.device).manual_seed(seed)
    m = s.w.shape[1]
    s.w.copy_(torch.linspace(0.5, 4.0, m, dtype=torch.float64, device=s.device)[None, :].expand(s.batch, -1))
    s.w[:, :6] = 1e-15
    for b in range(s.batch):
        s.v[b].normal_(generator=g).mul_(m ** -0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 300 and a batch of 4: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip
    from springcraft_amd.batch import DeviceBatchSolver
    from oracle.enm_oracle import synthetic_coord

    print(f"# tools/prs_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    ff = sc.InvariantForceField(13.0)
    print("# 1. one model, all non-trivial modes (ms)")
    print("#    N   k_mode_prs (events)   TFLOP/s   sc_modes_prs_subset (wall, with copy)   sc_modes_prs (wall, with copy)")
    for n in ((300,) if args.quick else (1000, 2000)):
        anm = sc.ANM(synthetic_coord(n, 1), ff)
        modes = anm._modes_device()
        rows = np.arange(6, 3 * n)
        old = wall_ms(lambda: modes.prs(1e-6, False), args.repeat)
        new = wall_ms(lambda: modes.prs_subset(rows, False), args.repeat)
        s = DeviceBatchSolver(n, 1, ff)
        fake_modes(torch, s, 0)
        ker = median_ms(torch, lambda: s.prs(norm=False), args.repeat)
        print(f"  {n:5d}   {ker:10.3f}   {tile_flops(n, 3 * n, 1) / ker * 1e-9:8.2f}   {new:10.3f}   {old:10.3f}")
        del s, anm, modes
        torch.cuda.empty_cache()

    batch, n = (4, 300) if args.quick else (64, 2000)
    print(f"# 2. {batch} x N = {n} (ms)")
    print("#    selection            prs(norm=False)   TFLOP/s   prs()   dcc(norm=False)")
    s = DeviceBatchSolver(n, batch, ff)
    s.matrix = None                                       # (nothing is solved here)
    torch.cuda.empty_cache()
    fake_modes(torch, s, 1)
    for name, subset, rows in (("all non-trivial modes", None, 3 * n), ("20 modes (6..25)", np.arange(6, 26), 20)):
        raw = median_ms(torch, lambda: s.prs(subset, norm=False), args.repeat)
        nrm = median_ms(torch, lambda: s.prs(subset), args.repeat)
        dcc = median_ms(torch, lambda: s.dcc(subset, norm=False), args.repeat)
        print(f"  {name:22s} {raw:10.3f}   {tile_flops(n, rows, batch) / raw * 1e-9:8.2f}   {nrm:10.3f}   {dcc:10.3f}")


if __name__ == "__main__":
    main()
