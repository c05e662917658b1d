"""
Timing of the pairwise comparison of mode subspaces (csrc/mode_subspace.hip) with stream events.

    python tools/subspace_timing.py [--quick] [--tile 32|64] [--skip-all-modes] > profiles/subspace.txt

1. 64 structures of N = 2000 (m = 6000), the k = 10 and k = 100 lowest non-trivial modes: rmsip and covariance_overlap of
   all 2080 pairs, next to dcc(norm=False) of the same selection on the same solver;
2. 8 structures of N = 2000 over the covariance rule's 5994 modes: covariance_overlap of the 36 pairs, next to
   dcc(norm=False).

The batch tensors are not solved: w is positive above six ~0 values and v random, which costs the kernels what eigenvectors
cost them.  Every figure is the median of `--repeat` runs after one warm-up, between two events on the solver's stream.
Bytes are those of v the kernel asks for -- per pair and tile 2 T rows of m doubles for the rows that carry a weight --
against the rate of a device-to-device copy measured here (read plus written bytes); flops are 2 per (pair, row pair,
column) as computed, whole T x T tiles, against the float64 matrix peak of 78.6 TFLOP/s.  `--tile` sets
SPRINGCRAFT_SUBSPACE_TILE before the library loads: the alternatives to the rule of subspace_tile().
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 78.6


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


def fake_modes(torch, s, seed):
    """Positive eigenvalues above six ~0 ones and random rows of unit length scale: nothing is solved."""
    g = torch.Generator(device=s.device).manual_seed(seed)
    m = s.w.shape[1]
    s.w.copy_(torch.linspace(0.5, 4.0, m, dtype=torch.float64, device=s.device)[None, :].expand(s.batch, -1))
    s.w[:, :6] = 1e-15
    for b in range(s.batch):
        s.v[b].normal_(generator=g).mul_(s.v.shape[2] ** -0.5)


def work(batch, k, m, tile):
    """(bytes of v asked for, flops as computed) of one self-comparison over k listed rows."""
    pairs = batch * (batch + 1) // 2
    tiles = -(-k // tile)
    return pairs * tiles * tiles * 2.0 * min(tile, k) * m * 8, pairs * tiles * tiles * 2.0 * tile * tile * m


def copy_rate(torch, device):
    x = torch.empty(1 << 27, dtype=torch.float64, device=device)     # 1 GiB
    y = torch.empty_like(x)
    ms = median_ms(torch, lambda: y.copy_(x), 5)
    return 2.0 * x.numel() * 8 / ms * 1e-9                             # TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 300 and batches of 4 / 2: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--tile", type=int, choices=(32, 64), default=None)
    ap.add_argument("--skip-all-modes", action="store_true", help="leave out workload 2")
    args = ap.parse_args()
    if args.tile:
        os.environ["SPRINGCRAFT_SUBSPACE_TILE"] = str(args.tile)
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip
    from springcraft_amd.batch import DeviceBatchSolver

    print(f"# tools/subspace_timing.py{' --quick' if args.quick else ''}{f' --tile {args.tile}' if args.tile else ''}: "
          f"{_hip.context().info()}")
    ff = sc.InvariantForceField(13.0)
    n = 300 if args.quick else 2000
    m = 3 * n
    rate = copy_rate(torch, torch.device("cuda", torch.cuda.current_device()))
    print(f"# device-to-device copy of 1 GiB: {rate:.2f} TB/s (read + written)")
    print("#   batch      k  tile   rmsip ms   cov_overlap ms    TB/s of v   of copy   TFLOP/s   of peak   dcc(norm=False) ms")

    def line(s, k, subset, cov_subset):
        tile = args.tile or (32 if k <= 32 else 64)
        byts, flops = work(s.batch, k, m, tile)
        cov = median_ms(torch, lambda: s.covariance_overlap(cov_subset), args.repeat)
        rms = median_ms(torch, lambda: s.rmsip(mode_subset=subset), args.repeat) if subset is not None else float("nan")
        dcc = median_ms(torch, lambda: s.dcc(cov_subset, norm=False), args.repeat)
        tbs, tf = byts / cov * 1e-9, flops / cov * 1e-9
        print(f"  {s.batch:6d} {k:6d} {tile:5d} {rms:10.3f} {cov:14.3f} {tbs:12.2f} {tbs / rate:9.2f} {tf:9.2f} "
              f"{tf / PEAK_TFLOPS:9.2f} {dcc:14.3f}", flush=True)

    s = DeviceBatchSolver(n, 4 if args.quick else 64, ff)
    s.matrix = None                                       # (nothing is solved here)
    torch.cuda.empty_cache()
    fake_modes(torch, s, 1)
    for k in (10, 100):
        rows = np.arange(6, 6 + k)
        line(s, k, rows, rows)
    del s
    torch.cuda.empty_cache()
    if not args.skip_all_modes:
        s = DeviceBatchSolver(n, 2 if args.quick else 8, ff)
        s.matrix = None
        torch.cuda.empty_cache()
        fake_modes(torch, s, 2)
        line(s, m - 6, None, None)                        # the covariance rule: every row but the six ~0 ones


if __name__ == "__main__":
    main()
