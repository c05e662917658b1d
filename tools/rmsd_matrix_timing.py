"""
Timing of the pairwise RMSD matrix (csrc/rmsd_matrix.hip) with stream events.

    python tools/rmsd_matrix_timing.py [--quick] [--ratios PYTEST_LOG] > profiles/rmsd_matrix.txt

1. Ensemble.rmsd_matrix() per call at M x N = 10000 x 2000, 2000 x 2000 and 200 x 50000, fit and no fit (no fit has no Jacobi:
   the difference is the epilogue), and at 2000 x 8 (all epilogue).  Flops are 18 per (pair, atom) over the whole 64 x 64
   tiles of the lower triangle and the atoms padded to 8, counted as computed; the fraction is of the float64 matrix rate
   (--peak, TFLOP/s).
2. The yardstick in the same run: prs(norm=False) of one structure of N = 2000 over all 6000 rows (csrc/mode_prs.hip, the
   same tile and MFMA schedule; fake modes as in tools/prs_timing.py), counted the same way.
3. The baseline the feature replaces: M successive Ensemble.rmsd(reference=f) calls at M = 2000, N = 2000, wall clock with
   one synchronisation at the end.
4. With --ratios: the largest measured / gate ratio of every group of comparisons in the output of
   ``pytest tests/test_rmsd_matrix_gpu.py -m gpu -s``.

Every event figure is the median of --repeat runs after one warm-up.
"""
import argparse
import os
import re
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


def tile_flops(side, length):
    t = -(-side // 64)
    return 18.0 * (t * (t + 1) // 2) * 4096 * length


def fake_modes(torch, s, seed):
    g = torch.Generator(device=s.device).manual_seed(seed)
    m = s.w.shape[1]
    s.w.copy_(torch.linspace(0.5, 4.0, m, dtype=torch.float64, device=s.device)[None, :].expand(s.batch, -1))
    s.w[:, :6] = 1e-15
    for b in range(s.batch):
        s.v[b].normal_(generator=g).mul_(m ** -0.5)


def frames_on_device(torch, m, n, seed):
    """Perturbed copies of one cloud of the size of a protein of n atoms, made on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.rand((1, n, 3), generator=g, dtype=torch.float64, device="cuda") * 5 * n ** (1 / 3)
    return base + 0.5 * torch.randn((m, n, 3), generator=g, dtype=torch.float64, device="cuda")


def ratios(path):
    groups = {}
    for line in open(path):
        m = re.match(r"\.*([^:]+): .*", line)
        found = re.findall(r"(?:= |ratio |allowed )(\d+\.\d+)", line)
        if not m or not found:
            continue
        label = m.group(1)
        key = ("against the model" if label.startswith("M=") else "other=" if label.startswith("other") else
               "non-finite frames" if label.startswith("NaN") else "rigid copies" if label.startswith("rigid") else
               "Ensemble.rmsd(reference=f)" if label.startswith("reference") else
               "host function" if label.startswith("host") else label)
        n, worst = groups.get(key, (0, 0.0))
        groups[key] = (n + 1, max(worst, max(float(v) for v in found)))
    print("# 4. largest measured / gate ratio per group of comparisons (tests/test_rmsd_matrix_gpu.py)")
    for key, (n, worst) in groups.items():
        print(f"  {key:30s} {n:4d} comparisons   {worst:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--peak", type=float, default=78.6, help="float64 matrix rate of the device, TFLOP/s")
    ap.add_argument("--ratios", help="output of pytest -s of the GPU tests, to summarise")
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip
    from springcraft_amd.batch import DeviceBatchSolver

    print(f"# tools/rmsd_matrix_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    print(f"# 1. Ensemble.rmsd_matrix(), ms per call (events); fraction of {args.peak} TFLOP/s")
    print("#      M        N      fit ms   TFLOP/s  fraction   no-fit ms   TFLOP/s  fraction")
    fractions = []
    shapes = ((300, 200), (200, 8)) if args.quick else ((10000, 2000), (2000, 2000), (200, 50000), (2000, 8))
    for m, n in shapes:
        ens = sc.Ensemble(frames_on_device(torch, m, n, 0))
        flops = tile_flops(m, -(-n // 8) * 8)
        fit = median_ms(torch, lambda: ens.rmsd_matrix(), args.repeat)
        raw = median_ms(torch, lambda: ens.rmsd_matrix(fit=False), args.repeat)
        tf, tr = flops / fit * 1e-9, flops / raw * 1e-9
        fractions.append(tf / args.peak)
        print(f"  {m:6d}   {n:6d}   {fit:9.3f}  {tf:8.2f}  {tf / args.peak:8.3f}   {raw:9.3f}  {tr:8.2f}  {tr / args.peak:8.3f}")
        del ens
        torch.cuda.empty_cache()

    n = 300 if args.quick else 2000
    print(f"# 2. yardstick: prs(norm=False), one structure of N = {n}, all {3 * n} rows (events)")
    s = DeviceBatchSolver(n, 1, sc.InvariantForceField(13.0))
    fake_modes(torch, s, 0)
    ker = median_ms(torch, lambda: s.prs(norm=False), args.repeat)
    tp = tile_flops(n, 3 * n) / ker * 1e-9
    print(f"  {ker:9.3f} ms   {tp:8.2f} TFLOP/s   fraction {tp / args.peak:.3f}")
    print(f"  rmsd_matrix(fit) at {shapes[0][0]} x {shapes[0][1]} reaches {fractions[0] / (tp / args.peak):.2f} of prs's fraction")
    del s
    torch.cuda.empty_cache()

    m, n = (100, 200) if args.quick else (2000, 2000)
    ens = sc.Ensemble(frames_on_device(torch, m, n, 1))
    for f in range(3):
        ens.rmsd(reference=f)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rows = [ens.rmsd(reference=f) for f in range(m)]
    torch.cuda.synchronize()
    loop = (time.perf_counter() - t) * 1e3
    one = median_ms(torch, lambda: ens.rmsd_matrix(), args.repeat)
    worst = float((torch.stack(rows, dim=1) - ens.rmsd_matrix()).abs().max())
    print(f"# 3. baseline at M = {m}, N = {n}: {m} calls of Ensemble.rmsd(reference=f) {loop:.1f} ms (wall), "
          f"one rmsd_matrix() {one:.3f} ms: {loop / one:.0f} x; largest difference of the two {worst:.2e}")
    if args.ratios:
        ratios(args.ratios)


if __name__ == "__main__":
    main()
