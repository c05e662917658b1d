"""
Cost of DeviceBatchSolver.anisotropic_fluctuation() against mean_square_fluctuation() on the same solved tensors; keep
the output as profiles/aniso_timing.txt.

  C3 shape:       N = 2000 ANM, full spectrum (6000 modes), --structures structures (64 = the benchmarked batch)
  low-mode shape: N = 2000 ANM, subset_by_index=(6, 25), 64 structures

Both consumers read the selected rows of v exactly once (selected rows x m x 8 bytes per structure), so the figure of
interest is the ratio of the two times; the achieved TB/s of each is given with its share of the 6.3 TB/s a streaming
read achieves on this chip.  The tensors keep six partial sums per atom and chunk where the MSF keeps three, and the
method adds the 6 -> 3x3 gather: the kernels alone (the C entry on a preallocated output) and the whole method are timed
separately.  Device events around --reps back-to-back calls, --runs times after a warm-up, the two consumers alternating
run by run; median and every run are printed.  No pass / fail.

Usage: python tools/aniso_timing.py [--structures B] [--atoms N] [--reps R] [--runs K] [--skip-full]
"""
import argparse
import ctypes as C
import json
import sys
from os.path import abspath, dirname

import numpy as np

sys.path.insert(0, dirname(dirname(abspath(__file__))))
import springcraft_amd as sc  # noqa: E402
from springcraft_amd import _hip  # noqa: E402
from springcraft_amd.batch import DeviceBatchSolver  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3


def coord_of(n_atoms, seed=0):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1 / 3)


def alternating_ms(torch, fns, reps, runs, warmup=2):
    """For every callable of `fns`: (median, runs) of the device time of `reps` back-to-back calls / reps; the callables
    take turns run by run, so that a drift of the clocks hits all of them alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    out = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return [(float(np.median(o)), [round(x, 4) for x in o]) for o in out]


def case(torch, label, n_atoms, batch, subset, reps, runs):
    s = DeviceBatchSolver(n_atoms, batch, sc.InvariantForceField(13.0), subset_by_index=subset)
    s.solve(torch.from_numpy(np.stack([coord_of(n_atoms, b) for b in range(batch)])).cuda())
    s.finish()
    nvec, m = s.w.shape[1], s.m
    row0 = max(6 - (subset[0] if subset else 0), 0)
    rows = nvec - row0
    u = s.anisotropic_fluctuation()
    msf = s.mean_square_fluctuation()
    trace = u.diagonal(dim1=-2, dim2=-1).sum(-1)
    rel = float(((trace - msf).abs() / msf.abs()).max())
    del u, trace, msf
    # the kernels alone: the C entry on a preallocated output, with the selection the method builds
    sel, counts = s._selection(None, pinv_default=False)
    out6 = torch.empty((batch, n_atoms, 6), dtype=torch.float64, device=s.device)
    L = _hip.lib()

    def kernels():
        s.ctx.check(L.sc_dev_modes_aniso_f64(s.ctx.handle, C.c_void_p(s.w.data_ptr()), C.c_void_p(s.v.data_ptr()), m, nvec,
                                             batch, C.byref(sel), counts, C.c_void_p(out6.data_ptr())))

    (a_ms, a_all), (k_ms, k_all), (f_ms, f_all) = alternating_ms(
        torch, [s.anisotropic_fluctuation, kernels, s.mean_square_fluctuation], reps, runs)
    nbytes = batch * rows * m * 8
    tbs = lambda ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731
    print(json.dumps({"case": label, "structures": batch, "rows": rows, "m": m, "bytes_read": nbytes,
                      "aniso_method_ms_median": round(a_ms, 4), "aniso_method_ms_runs": a_all,
                      "aniso_kernels_ms_median": round(k_ms, 4), "aniso_kernels_ms_runs": k_all,
                      "msf_method_ms_median": round(f_ms, 4), "msf_method_ms_runs": f_all,
                      "aniso_kernels_over_msf": round(k_ms / f_ms, 3), "aniso_method_over_msf": round(a_ms / f_ms, 3),
                      "aniso_kernels_TBps": round(tbs(k_ms), 3),
                      "aniso_kernels_share_of_6.3_TBps": round(tbs(k_ms) / HBM_ACHIEVABLE_TBS, 3),
                      "msf_TBps": round(tbs(f_ms), 3), "msf_share_of_6.3_TBps": round(tbs(f_ms) / HBM_ACHIEVABLE_TBS, 3),
                      "max_rel_diff_trace_to_msf": rel}), flush=True)
    del s, out6
    torch.cuda.empty_cache()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    args = ap.parse_args()
    n, b = args.atoms, args.structures
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv)}), flush=True)
    case(torch, f"low modes: {b} x N={n}, subset_by_index=(6, 25)", n, b, (6, 25), args.reps * 4, args.runs)
    if not args.skip_full:
        case(torch, f"C3 shape: {b} x N={n}, full spectrum", n, b, None, args.reps, args.runs)


if __name__ == "__main__":
    main()
