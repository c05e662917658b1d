"""
Cost of the batch consumers (DeviceBatchSolver.mean_square_fluctuation / .dcc) on the solver's own tensors.

  C3 shape:       N = 2000 ANM, full spectrum (6000 modes), --structures structures (64 = the benchmarked batch)
  low-mode shape: N = 2000 ANM, subset_by_index=(6, 25), 64 structures

MSF: device events around --reps calls, --runs times (median and spread over the runs); bytes read from the shapes
(selected rows x m x 8 per structure), achieved TB/s and its share of the 6.3 TB/s a streaming read achieves on this
chip.  Yardstick: what a user has today, the torch expression ((v * v) * s[:, :, None]).sum(1) folded over dim, in the
same process on the same tensors (s = 1 / w on the selected rows, 0 elsewhere).  The kernel must not be slower than that
beyond the spread measured here.
DCC (unnormalised): time, flops from the shapes (2 N^2 rows dim per structure), share of the f64 MFMA peak (78.6
TFLOP/s), and torch.bmm on the same packed operands as a reference point (C3 shape: as many structures at a time as the
1 GiB pack budget holds, i.e. one).  No pass / fail for DCC.

Usage: python tools/batch_consumers_timing.py [--structures B] [--reps R] [--runs K] [--skip-full]
"""
import argparse
import json
import sys
from os.path import abspath, dirname

import numpy as np

sys.path.insert(0, dirname(dirname(abspath(__file__))))
import springcraft_amd as sc  # noqa: E402
from springcraft_amd import _hip  # noqa: E402
from springcraft_amd.batch import DeviceBatchSolver  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3
F64_MFMA_PEAK_TFLOPS = 78.6


def coord_of(n_atoms, seed=0):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1 / 3)


def event_ms(torch, fn, reps, runs, warmup=2):
    """Median over `runs` of (device time of `reps` back-to-back calls) / reps, and every run's figure."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), [round(x, 4) for x in out]


def case(torch, label, n_atoms, batch, subset, reps, runs):
    dim = 3
    ff = sc.InvariantForceField(13.0)
    s = DeviceBatchSolver(n_atoms, batch, ff, subset_by_index=subset)
    s.solve(torch.from_numpy(np.stack([coord_of(n_atoms, b) for b in range(batch)])).cuda())
    s.finish()
    nvec, m = s.w.shape[1], s.m
    row0 = max(6 - (subset[0] if subset else 0), 0)
    rows = nvec - row0
    # ---- msf ----
    weights = torch.zeros_like(s.w)
    weights[:, row0:] = 1.0 / s.w[:, row0:]

    def torch_msf():
        return ((s.v * s.v) * weights[:, :, None]).sum(1).view(batch, n_atoms, dim).sum(2)

    ref, got = torch_msf(), s.mean_square_fluctuation()
    rel = float(((got - ref).abs() / ref.abs()).max())
    k_ms, k_all = event_ms(torch, s.mean_square_fluctuation, reps, runs)
    t_ms, t_all = event_ms(torch, torch_msf, max(1, reps // 4), runs)
    nbytes = batch * rows * m * 8
    tbs = nbytes / (k_ms * 1e-3) / 1e12
    spread = (max(k_all) - min(k_all)) + (max(t_all) - min(t_all))
    print(json.dumps({"case": label, "what": "msf", "structures": batch, "rows": rows, "m": m,
                      "kernel_ms_median": round(k_ms, 4), "kernel_ms_runs": k_all, "bytes_read": nbytes,
                      "achieved_TBps": round(tbs, 3), "share_of_6.3_TBps": round(tbs / HBM_ACHIEVABLE_TBS, 3),
                      "torch_expression_ms_median": round(t_ms, 4), "torch_expression_ms_runs": t_all,
                      "kernel_over_torch": round(k_ms / t_ms, 4), "spread_ms": round(spread, 4),
                      "not_slower_than_torch_beyond_spread": bool(k_ms <= t_ms + spread),
                      "max_rel_diff_to_torch": rel}), flush=True)
    del ref, got
    torch.cuda.empty_cache()
    # ---- dcc ----
    n = n_atoms
    flops = 2.0 * n * n * rows * dim * batch
    d_ms, d_all = event_ms(torch, lambda: s.dcc(norm=False, mode_subset=None if subset else np.arange(6, m)),
                           max(1, reps // 4), runs, warmup=1)
    # the same packed operands for the library: P (dim rows, N) per structure, S = P scaled by 1 / w
    per = 2 * rows * m * 8
    slab = max(1, min(batch, (1 << 30) // per))
    v = s.v[:slab, row0:]
    p = v.reshape(slab, rows, n, dim).permute(0, 3, 1, 2).reshape(slab, dim * rows, n).contiguous()
    sp = (p.view(slab, dim, rows, n) * weights[:slab, None, row0:, None]).view(slab, dim * rows, n)
    b_ms, b_all = event_ms(torch, lambda: torch.bmm(sp.transpose(1, 2), p), max(1, reps // 4), runs, warmup=1)
    b_ms_batch = b_ms * batch / slab
    print(json.dumps({"case": label, "what": "dcc (unnormalised)", "structures": batch, "rows": rows, "n_atoms": n,
                      "ms_median": round(d_ms, 3), "ms_runs": d_all, "flops": flops,
                      "achieved_TFLOPS": round(flops / (d_ms * 1e-3) / 1e12, 2),
                      "share_of_f64_mfma_peak": round(flops / (d_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS, 3),
                      "torch_bmm_structures_per_call": slab, "torch_bmm_ms_per_call_runs": b_all,
                      "torch_bmm_ms_scaled_to_batch": round(b_ms_batch, 3),
                      "torch_bmm_TFLOPS": round(flops / (b_ms_batch * 1e-3) / 1e12, 2),
                      "note": "torch.bmm times the product alone; dcc() also packs the operands"}), flush=True)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    args = ap.parse_args()
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv)}), flush=True)
    case(torch, "low modes: 64 x N=2000, subset_by_index=(6, 25)", 2000, 64, (6, 25), args.reps * 4, args.runs)
    if not args.skip_full:
        case(torch, f"C3 shape: {args.structures} x N=2000, full spectrum", 2000, args.structures, None, args.reps,
             args.runs)


if __name__ == "__main__":
    main()
